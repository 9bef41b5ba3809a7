// Micro-benchmark: what the FP4 MFMA of the matrix-core top-2 search (bf_mx.hip) costs the SIMD's vector issue, in MEASURED
// shader cycles (s_memtime, as cycles.hip).
//
// The body is the shipped group of 16 train rows: 8 x v_mfma_scale_f32_16x16x128_f8f6f4 cbsz:4 blgp:4 with VGPR accumulators -
// four that start from the threshold quads, four that accumulate in place - on operands held in registers (random FP4 +-1
// nibbles 0x2 / 0xA).  Three more FORMs of the same 8-MFMA body stand beside it: the unscaled spelling of the same shape
// (v_mfma_f32_16x16x128_f8f6f4), and the 32x32x64 shape, scaled by 2^0 and unscaled, as a group of 32 rows x 64 queries: two
// 32-query tiles x four K-quarters, the first quarter of a tile with C = inline 0, the rest accumulating in place, the tiles
// alternating.  A 32x32 MFMA does twice the MACs, so a group-equivalent (16 rows x 64 queries x 256 bits) is 8 MFMAs of the
// 16x16 forms and 4 of the 32x32 ones.
// Beside every MFMA go k = 0 .. 8 independent v_max3_i32 fillers (no register of an MFMA in them):
//   (i)   interleaved: k fillers after each MFMA, in the wave's own stream;
//   (ii)  bunched:     the 8 MFMAs, then 8 k fillers;
//   (iii) cross-wave:  the waves in even wave slots of a SIMD run bare groups, the waves in odd slots run ONLY fillers for a fixed
//                      1.5 M cycles of the shader clock - less than the MFMA waves need, so every filler counted was issued
//                      beside them - in bursts of 8 k with (4 - k) s_nop 15 between bursts (k = 4: back to back).
// at 2, 3 and 4 blocks per CU; the shipped form also at 1, and (iii), with k = 0 .. 4, at 2 and 4.  Every wave records where it ran (HW_ID, XCC_ID), so a row is computed per
// SIMD from the waves that really shared it: only SIMDs that held exactly the asked number of waves count, and the share of
// their span in which all of them ran is printed beside (waves of equal priority are served by age).  Per row: the SIMD's cycles per MFMA (its span / its MFMAs, median over SIMDs), an MFMA wave's
// own cycles per group, and for (iii) the fillers a filler wave issued per MFMA time of its SIMD.
// After each sweep over k a line fits the SIMD's cycles per MFMA to max(T, H + 4 k): T is the k = 0 row, H the mean of
// (cycles - 4 k) over the rows that lie a cycle or more above T, and the floor of a group-equivalent carrying the shipped
// 25.8 plain instructions is max(n T, n H + 4 x 25.8) with n = 8 or 4 MFMAs.
// It answers: how long an FP4 MFMA of either shape and spelling holds the vector issue, how many plain instructions per MFMA
// are free in-wave and cross-wave, and what the issue floor of the shipped mix is in each form.
// `mx_issue group [spin seconds]` runs instead the REAL group body of the 32x32x64 kernel (bf_mx32.hip) - the eight unscaled
// MFMAs on two accumulator sets, the two eight-instruction integer folds and one compare per tile, with the wait states the
// compiler puts between an MFMA and the first vector read of its result (11 after an 8-pass MFMA, every instruction between
// counting as one) - in four orders, at 1, 2, 3 and 4 waves per SIMD, and prints cycles per group and the share of the
// matrix pipe that is fed (8 x 32 cycles per group and wave):
//   (a) bunched:    t0k0 t1k0 t0k1 t1k1 t0k2 t1k2 t0k3 t1k3 | both folds                      (the order before the pipelined trip)
//   (b) pipelined:  t0k0 t0k1 [fold t1 of g - 1] t1k0 t1k1 t0k2 t1k2 t0k3 t1k3 [fold t0 of g]
//   (c) tile-major: t0k0 t0k1 [fold t1 of g - 1] t0k2 t0k3 t1k0 t1k1 [fold t0 of g] t1k2 t1k3 (four dependent MFMAs back to back)
//   (d) tile runs:  t0k0 t0k1 t0k2 t0k3 [fold t1 of g - 1] t1k0 t1k1 t1k2 t1k3 [fold t0 of g]  (each fold behind four MFMAs of the
//                   other tile and the other fold: the compiler owes no wait states; the order the kernel takes)
// `mx_issue fire [spin seconds]` runs the tile-run order (d) with a FIRED tile of the kernel's listing behind one fold of tile 0
// in every third group (one tile-group in six, 16.7 %; tools/mx_fire_model.py counts 17.7 % at the headline launch): the
// out-of-line block of gate compares, scalar tests, five vector instructions per entering row and the threshold tail, then a
// branch back.  Every fold ends, as in the kernel, in a compare into VCC, four moves and a branch; which fold fires, which gates
// are open and the threshold come from a table the kernel loads, k = 1, 2, 4 or 16 open rows ({6}, {3, 9}, {1, 5, 6, 12}, all).
// Five forms of the block, each at 1 .. 4 waves per SIMD, cycles per group and the share of the pipe fed as `group` prints:
//   (P)  the 16 row gates: 16 compares, 16 tests whose branch is TAKEN when the gate is closed, the open rows' bodies in line;
//   (A)  the fold as a tree whose first level is the maxima of five row groups ({0, 1, 14, 15}, {2, 3, 4}, ... {11, 12, 13}): 5
//        group compares and tests, and inside an open group its rows' compares and tests as in (P);
//   (B)  as (A), but all rows of an open group enter, no inner branch;
//   (F1) the 16 row gates with a closed gate falling through and every open row's body out of line, behind a label of its own;
//   (F2) the chain fold; the fired block computes four quad maxima (8 more vector instructions), then quad gates as in (A).
// It first prints the cycles of one s_cbranch_scc1, not taken and taken (to the next instruction), behind an s_cmp_eq_u32 that
// sets SCC from loaded values, less the cycles of the s_cmp alone.
// build: hipcc --offload-arch=gfx950 -O3 mx_issue.hip -o mx_issue
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <map>
#include <vector>
#define CK(x) do{hipError_t e=(x); if(e!=hipSuccess){printf("%s: %s\n",#x,hipGetErrorString(e)); return 1;}}while(0)

// registers of the 16x16 forms, as in the shipped listing: B operands v[2:33] (tile tt, K-half h at 2 + 8 tt + 4 h), threshold
// quads v[34:49], A operands v[50:53] / v[54:57], accumulators v[62:77].  Of the 32x32 forms: B operands v[2:33] (tile t,
// K-quarter q at 2 + 16 t + 4 q), A operands v[34:49] (quarter q at 34 + 4 q), accumulators v[50:65] and v[66:81].  The scales
// are in v96; the fillers use v[100:111] only
#define CLOB "v2","v3","v4","v5","v6","v7","v8","v9","v10","v11","v12","v13","v14","v15","v16","v17","v18","v19","v20","v21","v22","v23", \
             "v24","v25","v26","v27","v28","v29","v30","v31","v32","v33","v34","v35","v36","v37","v38","v39","v40","v41","v42","v43","v44","v45", \
             "v46","v47","v48","v49","v50","v51","v52","v53","v54","v55","v56","v57","v58","v59","v60","v61","v62","v63","v64","v65","v66","v67", \
             "v68","v69","v70","v71","v72","v73","v74","v75","v76","v77","v78","v79","v80","v81","v96","v100","v101","v102","v103","v104","v105", \
             "v106","v107","v108","v109","v110","v111"
#define SC ", v96, v96 op_sel_hi:[0,0,0] cbsz:4 blgp:4\n"
#define UN " cbsz:4 blgp:4\n"
#define MF(d, a, b, c) "v_mfma_scale_f32_16x16x128_f8f6f4 v[" d "], v[" a "], v[" b "], v[" c "]" SC
#define MU(d, a, b, c) "v_mfma_f32_16x16x128_f8f6f4 v[" d "], v[" a "], v[" b "], v[" c "]" UN
#define WF(d, a, b, c) "v_mfma_scale_f32_32x32x64_f8f6f4 v[" d "], v[" a "], v[" b "], " c SC
#define WU(d, a, b, c) "v_mfma_f32_32x32x64_f8f6f4 v[" d "], v[" a "], v[" b "], " c UN
#define F0 ""
#define F1 "v_max3_i32 v100, v108, v109, v110\n"
#define F2 F1 "v_max3_i32 v101, v109, v110, v111\n"
#define F3 F2 "v_max3_i32 v102, v110, v111, v108\n"
#define F4 F3 "v_max3_i32 v103, v111, v108, v109\n"
#define F5 F4 "v_max3_i32 v104, v108, v110, v109\n"
#define F6 F5 "v_max3_i32 v105, v109, v111, v110\n"
#define F7 F6 "v_max3_i32 v106, v110, v108, v111\n"
#define F8 F7 "v_max3_i32 v107, v111, v109, v108\n"
// the 8 MFMAs of a group, per form: A 16x16 scaled (shipped), B 16x16 unscaled, C 32x32 scaled, D 32x32 unscaled
#define A0 MF("62:65", "50:53", "2:5", "34:37")
#define A1 MF("66:69", "50:53", "10:13", "38:41")
#define A2 MF("70:73", "50:53", "18:21", "42:45")
#define A3 MF("74:77", "50:53", "26:29", "46:49")
#define A4 MF("62:65", "54:57", "6:9", "62:65")
#define A5 MF("66:69", "54:57", "14:17", "66:69")
#define A6 MF("70:73", "54:57", "22:25", "70:73")
#define A7 MF("74:77", "54:57", "30:33", "74:77")
#define B0 MU("62:65", "50:53", "2:5", "34:37")
#define B1 MU("66:69", "50:53", "10:13", "38:41")
#define B2 MU("70:73", "50:53", "18:21", "42:45")
#define B3 MU("74:77", "50:53", "26:29", "46:49")
#define B4 MU("62:65", "54:57", "6:9", "62:65")
#define B5 MU("66:69", "54:57", "14:17", "66:69")
#define B6 MU("70:73", "54:57", "22:25", "70:73")
#define B7 MU("74:77", "54:57", "30:33", "74:77")
#define C0 WF("50:65", "34:37", "2:5", "0")
#define C1 WF("66:81", "34:37", "18:21", "0")
#define C2 WF("50:65", "38:41", "6:9", "v[50:65]")
#define C3 WF("66:81", "38:41", "22:25", "v[66:81]")
#define C4 WF("50:65", "42:45", "10:13", "v[50:65]")
#define C5 WF("66:81", "42:45", "26:29", "v[66:81]")
#define C6 WF("50:65", "46:49", "14:17", "v[50:65]")
#define C7 WF("66:81", "46:49", "30:33", "v[66:81]")
#define D0 WU("50:65", "34:37", "2:5", "0")
#define D1 WU("66:81", "34:37", "18:21", "0")
#define D2 WU("50:65", "38:41", "6:9", "v[50:65]")
#define D3 WU("66:81", "38:41", "22:25", "v[66:81]")
#define D4 WU("50:65", "42:45", "10:13", "v[50:65]")
#define D5 WU("66:81", "42:45", "26:29", "v[66:81]")
#define D6 WU("50:65", "46:49", "14:17", "v[50:65]")
#define D7 WU("66:81", "46:49", "30:33", "v[66:81]")
// the real group body: folds of tile 0 (v[50:65] -> v100, compare into s[20:21]) and tile 1 (v[66:81] -> v101, s[22:23])
#define FD0 "v_max_i32 v100, v50, v51\n v_max3_i32 v100, v100, v52, v53\n v_max3_i32 v100, v100, v54, v55\n v_max3_i32 v100, v100, v56, v57\n" \
            "v_max3_i32 v100, v100, v58, v59\n v_max3_i32 v100, v100, v60, v61\n v_max3_i32 v100, v100, v62, v63\n v_max3_i32 v100, v100, v64, v65\n" \
            "v_cmp_ge_i32_e64 s[20:21], v100, v108\n"
#define FD1 "v_max_i32 v101, v66, v67\n v_max3_i32 v101, v101, v68, v69\n v_max3_i32 v101, v101, v70, v71\n v_max3_i32 v101, v101, v72, v73\n" \
            "v_max3_i32 v101, v101, v74, v75\n v_max3_i32 v101, v101, v76, v77\n v_max3_i32 v101, v101, v78, v79\n v_max3_i32 v101, v101, v80, v81\n" \
            "v_cmp_ge_i32_e64 s[22:23], v101, v109\n"
#define GROUP_A D0 D1 D2 D3 D4 D5 D6 D7 "s_nop 10\n" FD0 FD1
#define GROUP_B D0 D2 FD1 D1 D3 D4 D5 D6 D7 "s_nop 9\n" FD0
#define GROUP_C D0 D2 "s_nop 8\n" FD1 D4 D6 D1 D3 "s_nop 8\n" FD0 D5 D7
#define GROUP_D D0 D2 D4 D6 FD1 D1 D3 D5 D7 FD0
#define INTER_(P, F) P##0 F P##1 F P##2 F P##3 F P##4 F P##5 F P##6 F P##7 F
#define BUNCH_(P, F) P##0 P##1 P##2 P##3 P##4 P##5 P##6 P##7 F F F F F F F F
#define INTER_A(F) INTER_(A, F)
#define INTER_B(F) INTER_(B, F)
#define INTER_C(F) INTER_(C, F)
#define INTER_D(F) INTER_(D, F)
#define BUNCH_A(F) BUNCH_(A, F)
#define BUNCH_B(F) BUNCH_(B, F)
#define BUNCH_C(F) BUNCH_(C, F)
#define BUNCH_D(F) BUNCH_(D, F)
#define CLOBS CLOB, "s20", "s21", "s22", "s23"
#define NOP16 "s_nop 15\n"
#define X4(a) a a a a
#define FILL_CYCLES 1500000ull

// ---- the `fire` mode ----
// loaded per lane: the 16 row values v[112:127], the five group maxima v[82:86], the gates' threshold v87, the folds' quiet and
// firing thresholds v108 / v109.  Scratch: v[89:93] (tree / quad maxima), v[94:95], v[97:98] (the four moves), v102 / v103 (the
// sorted pair), v104 (key), v105 (base), v106 / v107 (threshold tail).  Gates: rows s[24:55], groups or quads s[56:65]
#define CLOBF CLOB, "v82","v83","v84","v85","v86","v87","v89","v90","v91","v92","v93","v94","v95","v97","v98","v112","v113","v114","v115", \
              "v116","v117","v118","v119","v120","v121","v122","v123","v124","v125","v126","v127","vcc","scc","s20","s21","s22","s23","s24", \
              "s25","s26","s27","s28","s29","s30","s31","s32","s33","s34","s35","s36","s37","s38","s39","s40","s41","s42","s43","s44","s45", \
              "s46","s47","s48","s49","s50","s51","s52","s53","s54","s55","s56","s57","s58","s59","s60","s61","s62","s63","s64","s65"
#define MOV4 "v_mov_b32 v94, v87\n v_mov_b32 v95, v102\n v_mov_b32 v97, v103\n v_mov_b32 v98, v107\n"
// the chain fold (the parent's) and the tree fold of a tile, compared against register T into VCC
#define CHAIN0(T) "v_max_i32 v100, v50, v51\n v_max3_i32 v100, v100, v52, v53\n v_max3_i32 v100, v100, v54, v55\n v_max3_i32 v100, v100, v56, v57\n" \
                  "v_max3_i32 v100, v100, v58, v59\n v_max3_i32 v100, v100, v60, v61\n v_max3_i32 v100, v100, v62, v63\n"                        \
                  "v_max3_i32 v100, v100, v64, v65\n v_cmp_ge_i32_e32 vcc, v100, " T "\n" MOV4
#define CHAIN1(T) "v_max_i32 v101, v66, v67\n v_max3_i32 v101, v101, v68, v69\n v_max3_i32 v101, v101, v70, v71\n v_max3_i32 v101, v101, v72, v73\n" \
                  "v_max3_i32 v101, v101, v74, v75\n v_max3_i32 v101, v101, v76, v77\n v_max3_i32 v101, v101, v78, v79\n"                        \
                  "v_max3_i32 v101, v101, v80, v81\n v_cmp_ge_i32_e32 vcc, v101, " T "\n" MOV4
#define TREE0(T) "v_max_i32 v89, v50, v51\n v_max3_i32 v90, v52, v53, v54\n v_max3_i32 v91, v55, v56, v57\n v_max3_i32 v92, v58, v59, v60\n" \
                 "v_max3_i32 v93, v61, v62, v63\n v_max3_i32 v89, v89, v64, v65\n v_max3_i32 v100, v90, v91, v92\n"                       \
                 "v_max3_i32 v100, v100, v93, v89\n v_cmp_ge_i32_e32 vcc, v100, " T "\n" MOV4
#define TREE1(T) "v_max_i32 v89, v66, v67\n v_max3_i32 v90, v68, v69, v70\n v_max3_i32 v91, v71, v72, v73\n v_max3_i32 v92, v74, v75, v76\n" \
                 "v_max3_i32 v93, v77, v78, v79\n v_max3_i32 v89, v89, v80, v81\n v_max3_i32 v101, v90, v91, v92\n"                       \
                 "v_max3_i32 v101, v101, v93, v89\n v_cmp_ge_i32_e32 vcc, v101, " T "\n" MOV4
// row i of a lane: X(two-digit index, its value's register, its gate's SGPR pair, its offset 8 (i >> 2) + (i & 3))
#define R0(X) X("00", "112", "24", "25", "0")
#define R1(X) X("01", "113", "26", "27", "1")
#define R2(X) X("02", "114", "28", "29", "2")
#define R3(X) X("03", "115", "30", "31", "3")
#define R4(X) X("04", "116", "32", "33", "8")
#define R5(X) X("05", "117", "34", "35", "9")
#define R6(X) X("06", "118", "36", "37", "10")
#define R7(X) X("07", "119", "38", "39", "11")
#define R8(X) X("08", "120", "40", "41", "16")
#define R9(X) X("09", "121", "42", "43", "17")
#define R10(X) X("10", "122", "44", "45", "18")
#define R11(X) X("11", "123", "46", "47", "19")
#define R12(X) X("12", "124", "48", "49", "24")
#define R13(X) X("13", "125", "50", "51", "25")
#define R14(X) X("14", "126", "52", "53", "26")
#define R15(X) X("15", "127", "54", "55", "27")
#define ROWS_ALL(X) R0(X) R1(X) R2(X) R3(X) R4(X) R5(X) R6(X) R7(X) R8(X) R9(X) R10(X) R11(X) R12(X) R13(X) R14(X) R15(X)
#define ROWS_G0(X) R0(X) R1(X) R14(X) R15(X)
#define ROWS_G1(X) R2(X) R3(X) R4(X)
#define ROWS_G2(X) R5(X) R6(X) R7(X)
#define ROWS_G3(X) R8(X) R9(X) R10(X)
#define ROWS_G4(X) R11(X) R12(X) R13(X)
#define ROWS_Q0(X) R0(X) R1(X) R2(X) R3(X)
#define ROWS_Q1(X) R4(X) R5(X) R6(X) R7(X)
#define ROWS_Q2(X) R8(X) R9(X) R10(X) R11(X)
#define ROWS_Q3(X) R12(X) R13(X) R14(X) R15(X)
// the five vector instructions of an entering row: key = base + offset - (D << 22), into the sorted pair
#define BODY(v, off) "v_cvt_i32_f32_e64 v104, -v" v "\n v_lshlrev_b32 v104, 22, v104\n v_add3_u32 v104, v105, v104, " off "\n"  \
                     "v_med3_u32 v103, v102, v103, v104\n v_min_u32 v102, v102, v104\n"
#define XCMP(i, v, sl, sh, off) "v_cmp_ge_i32_e64 s[" sl ":" sh "], v" v ", v87\n"
#define XGATED(i, v, sl, sh, off) "s_cmp_eq_u64 s[" sl ":" sh "], 0\n s_cbranch_scc1 1" i "f\n" BODY(v, off) "1" i ":\n"
#define XBODY(i, v, sl, sh, off) BODY(v, off)
#define XTEST_OUT(i, v, sl, sh, off) "s_cmp_lg_u64 s[" sl ":" sh "], 0\n s_cbranch_scc1 2" i "f\n 3" i ":\n"
#define XBODY_OUT(i, v, sl, sh, off) "2" i ":\n" BODY(v, off) "s_branch 3" i "b\n"
// gate j of the groups (value in register g) or quads: compare, and the test that skips to label 40j
#define GCMP(j, g) "v_cmp_ge_i32_e64 s[" j "], " g ", v87\n"
#define GCMPS GCMP("56:57", "v82") GCMP("58:59", "v83") GCMP("60:61", "v84") GCMP("62:63", "v85") GCMP("64:65", "v86")
#define GTEST(j, n) "s_cmp_eq_u64 s[" j "], 0\n s_cbranch_scc1 40" n "f\n"
#define OPEN_A(j, n, ROWS) GTEST(j, n) ROWS(XCMP) ROWS(XGATED) "40" n ":\n"
#define OPEN_B(j, n, ROWS) GTEST(j, n) ROWS(XBODY) "40" n ":\n"
#define QUADS "v_max3_i32 v89, v112, v113, v114\n v_max3_i32 v90, v116, v117, v118\n v_max3_i32 v91, v120, v121, v122\n"                    \
              "v_max3_i32 v92, v124, v125, v126\n v_max_i32 v89, v89, v115\n v_max_i32 v90, v90, v119\n v_max_i32 v91, v91, v123\n"          \
              "v_max_i32 v92, v92, v127\n" GCMP("56:57", "v89") GCMP("58:59", "v90") GCMP("60:61", "v91") GCMP("62:63", "v92")
#define BLOCK_P ROWS_ALL(XCMP) ROWS_ALL(XGATED)
#define BLOCK_A GCMPS OPEN_A("56:57", "0", ROWS_G0) OPEN_A("58:59", "1", ROWS_G1) OPEN_A("60:61", "2", ROWS_G2) OPEN_A("62:63", "3", ROWS_G3) \
                OPEN_A("64:65", "4", ROWS_G4)
#define BLOCK_B GCMPS OPEN_B("56:57", "0", ROWS_G0) OPEN_B("58:59", "1", ROWS_G1) OPEN_B("60:61", "2", ROWS_G2) OPEN_B("62:63", "3", ROWS_G3) \
                OPEN_B("64:65", "4", ROWS_G4)
#define BLOCK_F1 ROWS_ALL(XCMP) ROWS_ALL(XTEST_OUT)
#define BLOCK_F2 QUADS OPEN_A("56:57", "0", ROWS_Q0) OPEN_A("58:59", "1", ROWS_Q1) OPEN_A("60:61", "2", ROWS_Q2) OPEN_A("62:63", "3", ROWS_Q3)
// the threshold tail: seven dependent vector instructions and an s_nop
#define TAIL "v_lshrrev_b32 v106, 23, v103\n v_min_u32 v107, v107, v106\n v_lshlrev_b32 v106, 1, v107\n v_sub_u32 v106, 0x102, v106\n" \
             "v_cvt_f32_u32 v106, v106\n v_cmp_gt_u32_e32 vcc, 0x82, v107\n s_nop 0\n v_cndmask_b32 v106, v105, v106, vcc\n"
// three groups in the order (d); the fold of tile 0 of the second fires.  The fired block (label 2) and the out-of-line row
// bodies stand in front of the groups; a quiet fold's branch is never taken
#define BRQ "s_cbranch_vccnz 2b\n"
#define FIRE_LOOP(F0, F1, BLOCK, OUTLINE)                                                                      \
    "s_branch 1f\n 2:\n" BLOCK TAIL "s_branch 3f\n" OUTLINE "1:\n"                                             \
    D0 D2 D4 D6 F1("v108") BRQ D1 D3 D5 D7 F0("v108") BRQ                                                      \
    D0 D2 D4 D6 F1("v108") BRQ D1 D3 D5 D7 F0("v109") "s_cbranch_vccnz 2b\n 3:\n"                              \
    D0 D2 D4 D6 F1("v108") BRQ D1 D3 D5 D7 F0("v108") BRQ
#define FIRE_ROWS 24                                   // ints per lane of the table

struct stamp { unsigned long long c0, r0, c1, r1; unsigned role, hwid, xcc, count; };

// FORM 0 16x16x128 scaled (shipped) | 1 16x16x128 unscaled | 2 32x32x64 scaled | 3 32x32x64 unscaled | 4, 5, 6, 7 the real group
// body of the 32x32x64 kernel in the orders (a), (b), (c), (d) (PLACE 0, K 0);
// PLACE 0 interleaved | 1 bunched | 2 cross-wave; K fillers per MFMA
#define PICK(BODY)                                            \
    {                                                         \
        if (K == 0) asm volatile(X4(BODY(F0)) ::: CLOB);      \
        if (K == 1) asm volatile(X4(BODY(F1)) ::: CLOB);      \
        if (K == 2) asm volatile(X4(BODY(F2)) ::: CLOB);      \
        if (K == 3) asm volatile(X4(BODY(F3)) ::: CLOB);      \
        if (K == 4) asm volatile(X4(BODY(F4)) ::: CLOB);      \
        if (K == 5) asm volatile(X4(BODY(F5)) ::: CLOB);      \
        if (K == 6) asm volatile(X4(BODY(F6)) ::: CLOB);      \
        if (K == 7) asm volatile(X4(BODY(F7)) ::: CLOB);      \
        if (K == 8) asm volatile(X4(BODY(F8)) ::: CLOB);      \
    }
template <int FORM, int PLACE, int K>
__global__ __launch_bounds__(256) void k(uint32_t* out, stamp* st, int iters, const int* gd) {
    static_assert(PLACE < 2 || (FORM == 0 && K <= 4), "the cross-wave rows exist for the shipped form only");
    uint32_t seed = threadIdx.x * 2654435761u + blockIdx.x * 40503u + 1u;
    // FP4 +-1 operands: every nibble 0x2 or 0xA
#define RND(r) "v_mul_lo_u32 %0, %0, %1\n v_and_b32 " r ", 0x88888888, %0\n v_or_b32 " r ", 0x22222222, " r "\n"
    asm volatile(RND("v2") RND("v3") RND("v4") RND("v5") RND("v6") RND("v7") RND("v8") RND("v9") RND("v10") RND("v11") RND("v12") RND("v13")
                 RND("v14") RND("v15") RND("v16") RND("v17") RND("v18") RND("v19") RND("v20") RND("v21") RND("v22") RND("v23") RND("v24")
                 RND("v25") RND("v26") RND("v27") RND("v28") RND("v29") RND("v30") RND("v31") RND("v32") RND("v33") RND("v34") RND("v35")
                 RND("v36") RND("v37") RND("v38") RND("v39") RND("v40") RND("v41") RND("v42") RND("v43") RND("v44") RND("v45") RND("v46")
                 RND("v47") RND("v48") RND("v49") RND("v50") RND("v51") RND("v52") RND("v53") RND("v54") RND("v55") RND("v56") RND("v57")
                 : "+v"(seed) : "v"(1664525u) : CLOB);
    // fillers' inputs, scale 2^0 on both sides
    asm volatile("v_mov_b32 v108, %0\n v_mov_b32 v109, %0\n v_mov_b32 v110, %0\n v_mov_b32 v111, %0\n v_mov_b32 v100, 0\n v_mov_b32 v101, 0\n"
                 "v_mov_b32 v102, 0\n v_mov_b32 v103, 0\n v_mov_b32 v104, 0\n v_mov_b32 v105, 0\n v_mov_b32 v106, 0\n v_mov_b32 v107, 0\n"
                 "v_mov_b32 v96, 0x7f7f7f7f\n" ::"v"(seed) : CLOB);
    // the 16x16 forms: thresholds as in the kernel (2 x - 258 for some x) where the 32x32 forms keep A operands
    if (FORM < 2)
        asm volatile("v_mov_b32 v34, 0xc2a00000\n v_mov_b32 v35, v34\n v_mov_b32 v36, v34\n v_mov_b32 v37, v34\n v_mov_b32 v38, v34\n v_mov_b32 v39, v34\n"
                     "v_mov_b32 v40, v34\n v_mov_b32 v41, v34\n v_mov_b32 v42, v34\n v_mov_b32 v43, v34\n v_mov_b32 v44, v34\n v_mov_b32 v45, v34\n"
                     "v_mov_b32 v46, v34\n v_mov_b32 v47, v34\n v_mov_b32 v48, v34\n v_mov_b32 v49, v34\n" A0 A1 A2 A3 "s_nop 15\n" ::: CLOB);
    else
        asm volatile(C0 C1 "s_nop 15\n s_nop 15\n" ::: CLOB);
    if (FORM >= 8) {                                    // the fire mode's table, lane by lane
        const uint32_t off = (threadIdx.x & 63) * FIRE_ROWS * 4;
        asm volatile("global_load_dwordx4 v[112:115], %0, %1\n global_load_dwordx4 v[116:119], %0, %1 offset:16\n"
                     "global_load_dwordx4 v[120:123], %0, %1 offset:32\n global_load_dwordx4 v[124:127], %0, %1 offset:48\n"
                     "global_load_dwordx4 v[82:85], %0, %1 offset:64\n global_load_dwordx2 v[86:87], %0, %1 offset:80\n"
                     "global_load_dwordx2 v[108:109], %0, %1 offset:88\n s_waitcnt vmcnt(0)\n"
                     "v_mov_b32 v105, 0x40000000\n v_mov_b32 v102, -1\n v_mov_b32 v103, -1\n v_mov_b32 v107, 0x1ff" ::"v"(off), "s"(gd) : CLOBF);
    }
    unsigned hwid, xcc, count = 0;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)\n s_getreg_b32 %1, hwreg(HW_REG_XCC_ID)" : "=s"(hwid), "=s"(xcc));
    const bool filler_wave = PLACE == 2 && (hwid & 1);             // HW_ID[3:0] = wave slot of the SIMD
    unsigned long long c0, r0, c1, r1;
    asm volatile("s_memtime %0\n s_memrealtime %1\n s_waitcnt lgkmcnt(0)" : "=s"(c0), "=s"(r0)::"memory");
    if (!filler_wave) {
        for (int it = 0; it < iters; it += FORM >= 8 ? 3 : 4) {
            if (FORM == 8) asm volatile(FIRE_LOOP(CHAIN0, CHAIN1, BLOCK_P, "") ::: CLOBF);
            else if (FORM == 9) asm volatile(FIRE_LOOP(TREE0, TREE1, BLOCK_A, "") ::: CLOBF);
            else if (FORM == 10) asm volatile(FIRE_LOOP(TREE0, TREE1, BLOCK_B, "") ::: CLOBF);
            else if (FORM == 11) asm volatile(FIRE_LOOP(CHAIN0, CHAIN1, BLOCK_F1, ROWS_ALL(XBODY_OUT)) ::: CLOBF);
            else if (FORM == 12) asm volatile(FIRE_LOOP(CHAIN0, CHAIN1, BLOCK_F2, "") ::: CLOBF);
            else if (PLACE == 2) asm volatile(X4(INTER_A(F0)) ::: CLOB);
            else if (FORM == 0 && PLACE == 0) PICK(INTER_A)
            else if (FORM == 0 && PLACE == 1) PICK(BUNCH_A)
            else if (FORM == 1 && PLACE == 0) PICK(INTER_B)
            else if (FORM == 1 && PLACE == 1) PICK(BUNCH_B)
            else if (FORM == 2 && PLACE == 0) PICK(INTER_C)
            else if (FORM == 2 && PLACE == 1) PICK(BUNCH_C)
            else if (FORM == 3 && PLACE == 0) PICK(INTER_D)
            else if (FORM == 3 && PLACE == 1) PICK(BUNCH_D)
            else if (FORM == 4) asm volatile(X4(GROUP_A) ::: CLOBS);
            else if (FORM == 5) asm volatile(X4(GROUP_B) ::: CLOBS);
            else if (FORM == 6) asm volatile(X4(GROUP_C) ::: CLOBS);
            else if (FORM == 7) asm volatile(X4(GROUP_D) ::: CLOBS);
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
    asm volatile("s_nop 15\n s_nop 15\n v_add_u32 %0, v62, v66\n v_add_u32 %0, %0, v70\n v_add_u32 %0, %0, v74\n v_add_u32 %0, %0, v100\n v_add_u32 %0, %0, v101\n"
                 "v_add_u32 %0, %0, v102\n v_add_u32 %0, %0, v103\n v_add_u32 %0, %0, v104\n v_add_u32 %0, %0, v105\n v_add_u32 %0, %0, v106\n"
                 "v_add_u32 %0, %0, v107" : "=v"(s)::CLOB);
    out[blockIdx.x * 256 + threadIdx.x] = s;
    if ((threadIdx.x & 63) == 0) {
        stamp v = {c0, r0, c1, r1, filler_wave ? 1u : 0u, hwid, xcc, count};
        st[blockIdx.x * 4 + (threadIdx.x >> 6)] = v;
    }
}

static double median(std::vector<double>& v) { std::sort(v.begin(), v.end()); return v.empty() ? 0.0 : v[v.size() / 2]; }

static const int MAXW = 4, NCU = 256;
static const char* const FORM_NAME[] = {"16x16x128 scaled", "16x16x128 plain ", "32x32x64 scaled ", "32x32x64 plain  ",
                                        "group (a) bunched", "group (b) pipelined", "group (c) tile-major", "group (d) tile runs",
                                        "fire (P) 16 row gates", "fire (A) 5 groups, row gates", "fire (B) 5 groups, rows enter",
                                        "fire (F1) open rows out of line", "fire (F2) quads in the block"};

// one row; *cyc = the SIMD's cycles per MFMA (median over SIMDs)
template <int FORM, int PLACE, int K> int run(int waves, uint32_t* out, stamp* d_st, double spin_s, double* cyc, const int* gd = nullptr) {
    const int iters = FORM >= 8 ? 19998 : 20000, blocks = NCU * waves;   // the fire mode's loop is three groups
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    CK(hipEventRecord(e0));
    float spun = 0;
    while (spun < spin_s * 1e3f) {                      // spin-up: back-to-back launches of the same body
        for (int i = 0; i < 8; i++) k<FORM, PLACE, K><<<blocks, 256>>>(out, d_st, iters, gd);
        CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1));
        CK(hipEventElapsedTime(&spun, e0, e1));
    }
    k<FORM, PLACE, K><<<blocks, 256>>>(out, d_st, iters, gd);
    CK(hipDeviceSynchronize());
    CK(hipEventDestroy(e0)); CK(hipEventDestroy(e1));
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
    *cyc = median(per_mfma);
    printf("%s %-11s k %d  blocks/CU %d: %4zu of %4zu SIMDs held %d waves, all running for %3.0f %% of the span | %6.2f cycles/MFMA/SIMD | an MFMA "
           "wave's own group: p10 %6.1f median %6.1f p90 %6.1f cycles",
           FORM_NAME[FORM], place[PLACE], K, waves, used, simd.size(), waves, 100 * median(together), *cyc, grp[grp.size() / 10], median(grp),
           grp[grp.size() * 9 / 10]);
    if (PLACE == 2 && K) printf(" | fillers issued beside the MFMAs: %5.2f per MFMA time", median(fill_per_mfma));
    printf(" | clock %4.0f MHz\n", mclk);
    fflush(stdout);
    return 0;
}

// the fit of max(T, H + 4 k) to the rows k = 0 .. 8 of one form and placement, and the issue floor of a group-equivalent
static void fit(int form, int place, int waves, const double* c) {
    double h = 0;
    int n = 0;
    for (int kk = 1; kk <= 8; kk++)
        if (c[kk] >= c[0] + 1.0) { h += c[kk] - 4.0 * kk; n++; }
    const int per_group = form < 2 ? 8 : 4;
    if (n) {
        h /= n;
        printf("  fit %s %-11s blocks/CU %d: T %6.2f  H %6.2f (mean of cycles - 4 k over %d rows above T + 1) | group-equivalent of %d MFMAs + "
               "25.8 plain: max(%5.1f, %5.1f) = %5.1f cycles\n",
               FORM_NAME[form], place ? "bunched" : "interleaved", waves, c[0], h, n, per_group, per_group * c[0], per_group * h + 4 * 25.8,
               std::max(per_group * c[0], per_group * h + 4 * 25.8));
    } else {
        printf("  fit %s %-11s blocks/CU %d: T %6.2f  no row above T + 1: H <= %6.2f | group-equivalent of %d MFMAs: %5.1f cycles\n",
               FORM_NAME[form], place ? "bunched" : "interleaved", waves, c[0], c[0] - 32.0, per_group, per_group * c[0]);
    }
    fflush(stdout);
}

// k = 0 .. 8 of one form and placement and their fit; the cross-wave rows stop at k = 4 and have none
template <int FORM, int PLACE> int sweep(int waves, uint32_t* out, stamp* d_st, double spin_s) {
    double c[9] = {};
    if (run<FORM, PLACE, 0>(waves, out, d_st, spin_s, c + 0)) return 1;
    if (run<FORM, PLACE, 1>(waves, out, d_st, spin_s, c + 1)) return 1;
    if (run<FORM, PLACE, 2>(waves, out, d_st, spin_s, c + 2)) return 1;
    if (run<FORM, PLACE, 3>(waves, out, d_st, spin_s, c + 3)) return 1;
    if (run<FORM, PLACE, 4>(waves, out, d_st, spin_s, c + 4)) return 1;
    if constexpr (PLACE < 2) {
        if (run<FORM, PLACE, 5>(waves, out, d_st, spin_s, c + 5)) return 1;
        if (run<FORM, PLACE, 6>(waves, out, d_st, spin_s, c + 6)) return 1;
        if (run<FORM, PLACE, 7>(waves, out, d_st, spin_s, c + 7)) return 1;
        if (run<FORM, PLACE, 8>(waves, out, d_st, spin_s, c + 8)) return 1;
        fit(FORM, PLACE, waves, c);
    }
    return 0;
}

template <int FORM> int form(uint32_t* out, stamp* d_st, double spin_s) {
    for (int w : {2, 3, 4}) {
        if (sweep<FORM, 0>(w, out, d_st, spin_s)) return 1;
        if (sweep<FORM, 1>(w, out, d_st, spin_s)) return 1;
    }
    return 0;
}

// the real group body in one order at 1 .. 4 waves per SIMD: cycles per group and SIMD, and the share of the pipe that is fed
template <int FORM> int group_rows(uint32_t* out, stamp* d_st, double spin_s) {
    for (int w : {1, 2, 3, 4}) {
        double c = 0;
        if (run<FORM, 0, 0>(w, out, d_st, spin_s, &c)) return 1;
        printf("  %s, %d waves per SIMD: %6.1f cycles per group and SIMD, pipe fed %5.1f %%\n", FORM_NAME[FORM], w, 8 * c, 100.0 * 32.0 / c);
        fflush(stdout);
    }
    return 0;
}

// the fire mode's table for k open rows: the open rows hold 200 in lane 5 and 0 elsewhere, the threshold is 100 in every lane
static void fire_table(int k, std::vector<int>& t) {
    static const int one[] = {6}, two[] = {3, 9}, four[] = {1, 5, 6, 12};
    static const int groups[5][4] = {{0, 1, 14, 15}, {2, 3, 4, -1}, {5, 6, 7, -1}, {8, 9, 10, -1}, {11, 12, 13, -1}};
    t.assign(64 * FIRE_ROWS, 0);
    for (int lane = 0; lane < 64; lane++) {
        int* r = t.data() + lane * FIRE_ROWS;
        if (lane == 5)
            for (int i = 0; i < k; i++) r[k == 16 ? i : k == 4 ? four[i] : k == 2 ? two[i] : one[i]] = 200;
        for (int j = 0; j < 5; j++)
            for (int i : groups[j])
                if (i >= 0) r[16 + j] = std::max(r[16 + j], r[i]);
        r[21] = 100;
        r[22] = 0x7fffffff;                             // a quiet fold's threshold: above every pattern
        r[23] = (int)0x80000000u;                       // the firing fold's: below every pattern
    }
}

template <int FORM> int fire_rows(uint32_t* out, stamp* d_st, double spin_s, int* gd) {
    for (int k : {1, 2, 4, 16}) {
        std::vector<int> t;
        fire_table(k, t);
        CK(hipMemcpy(gd, t.data(), t.size() * sizeof(int), hipMemcpyHostToDevice));
        for (int w : {1, 2, 3, 4}) {
            double c = 0;
            if (run<FORM, 0, 0>(w, out, d_st, spin_s, &c, gd)) return 1;
            printf("  %s, k = %2d open rows, %d waves per SIMD: %6.1f cycles per group and SIMD, pipe fed %5.1f %%\n", FORM_NAME[FORM], k, w, 8 * c,
                   100.0 * 32.0 / c);
            fflush(stdout);
        }
    }
    return 0;
}

// 256 x (s_cmp_eq_u32 of two loaded values [+ s_cbranch_scc1 to the next instruction]) per trip: a dependent chain through SCC
#define X16(a) X4(X4(a))
#define X256(a) X16(X16(a))
template <bool BRANCH> __global__ void kb(unsigned long long* cyc, const int* v, int trips) {
    const int a = v[0], b = v[1];
    unsigned long long c0, c1;
    asm volatile("s_memtime %0\n s_waitcnt lgkmcnt(0)" : "=s"(c0)::"memory");
    for (int i = 0; i < trips; i++) {
        if (BRANCH) asm volatile(X256("s_cmp_eq_u32 %0, %1\n s_cbranch_scc1 1f\n 1:\n") ::"s"(a), "s"(b) : "scc");
        else asm volatile(X256("s_cmp_eq_u32 %0, %1\n") ::"s"(a), "s"(b) : "scc");
    }
    asm volatile("s_memtime %0\n s_waitcnt lgkmcnt(0)" : "=s"(c1)::"memory");
    if (threadIdx.x == 0) cyc[blockIdx.x] = c1 - c0;
}

static int branch_rows(int* gd) {
    const int trips = 1000;
    unsigned long long* d; CK(hipMalloc(&d, NCU * sizeof(*d)));
    double res[3];
    for (int mode = 0; mode < 3; mode++) {                // 0 the compare alone | 1 branch not taken | 2 branch taken
        const int v[2] = {1, mode == 2 ? 1 : 2};
        CK(hipMemcpy(gd, v, sizeof(v), hipMemcpyHostToDevice));
        for (int rep = 0; rep < 3; rep++) {
            if (mode) kb<true><<<NCU, 64>>>(d, gd, trips);
            else kb<false><<<NCU, 64>>>(d, gd, trips);
        }
        CK(hipDeviceSynchronize());
        std::vector<unsigned long long> h(NCU);
        CK(hipMemcpy(h.data(), d, NCU * sizeof(*d), hipMemcpyDeviceToHost));
        std::vector<double> c;
        for (auto x : h) c.push_back((double)x / (256.0 * trips));
        res[mode] = median(c);
    }
    printf("  one wave per CU, a chain of 256000: s_cmp_eq_u32 alone %5.2f cycles | + s_cbranch_scc1 not taken %5.2f (branch %5.2f) | + "
           "s_cbranch_scc1 taken to the next instruction %5.2f (branch %5.2f)\n", res[0], res[1], res[1] - res[0], res[2], res[2] - res[0]);
    fflush(stdout);
    CK(hipFree(d));
    return 0;
}

int main(int argc, char** argv) {
    const bool group = argc > 1 && !strcmp(argv[1], "group");
    const bool fire = argc > 1 && !strcmp(argv[1], "fire");
    const double spin_s = argc > 1 + (group || fire) ? atof(argv[1 + (group || fire)]) : 0.5;
    uint32_t* out; CK(hipMalloc(&out, (size_t)NCU * MAXW * 256 * 4));
    stamp* d_st; CK(hipMalloc(&d_st, (size_t)NCU * MAXW * 4 * sizeof(stamp)));
    if (fire) {
        int* gd; CK(hipMalloc(&gd, 64 * FIRE_ROWS * sizeof(int)));
        return branch_rows(gd) || fire_rows<8>(out, d_st, spin_s, gd) || fire_rows<9>(out, d_st, spin_s, gd) ||
               fire_rows<10>(out, d_st, spin_s, gd) || fire_rows<11>(out, d_st, spin_s, gd) || fire_rows<12>(out, d_st, spin_s, gd);
    }
    if (group) return group_rows<4>(out, d_st, spin_s) || group_rows<5>(out, d_st, spin_s) || group_rows<6>(out, d_st, spin_s) ||
                      group_rows<7>(out, d_st, spin_s);
    if (form<0>(out, d_st, spin_s) || form<1>(out, d_st, spin_s) || form<2>(out, d_st, spin_s) || form<3>(out, d_st, spin_s)) return 1;
    // the shipped form alone on its SIMD, and beside waves that issue only fillers
    if (sweep<0, 0>(1, out, d_st, spin_s) || sweep<0, 1>(1, out, d_st, spin_s)) return 1;
    if (sweep<0, 2>(2, out, d_st, spin_s) || sweep<0, 2>(4, out, d_st, spin_s)) return 1;
    return 0;
}
