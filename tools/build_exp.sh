#!/bin/bash
# Builds the two experiment variants of libslamhip.so used by tools/trace_probe.py and tools/exp_probe.py into
# tools/exp/ (development aid; nothing in the product or the tests loads them).  Both are the shipped sources with a
# small patch applied to a temporary copy of bf_hamming.hip:
#   libslamhip_trace.so      every block stamps wall_clock64() at start / after the prologue / after the scan / at the end,
#                            and where it runs (HW_REG_HW_ID, HW_REG_XCC_ID), behind the stamps
#   libslamhip_keepbound.so  the last arriver leaves the final 2nd-best distance in bound[] instead of restoring it
#   libslamhip_count.so      counts, per launch, the 16-row groups and the single rows that take the update path
#   libslamhip_cycles.so     wave 0 of every block stamps s_memtime (shader cycles) AND s_memrealtime (100 MHz) at block
#                            start / after the prologue / after the scan / at the end, into a buffer of its own
set -euo pipefail
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
SRC="$ROOT/slam-experiments_amd/csrc"
OUT="$ROOT/tools/exp"
TMP="$(mktemp -d)"
mkdir -p "$OUT"
make -C "$SRC" -j8 all >/dev/null
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -I$ROOT/include -I/opt/rocm/include -I$SRC -fvisibility=hidden -DSLAM_BUILD"

# tools/build_exp.sh orb-mutants: six copies of the library, each with ONE deliberate mistake in a temporary copy of orb.hip
# (comparisons and constants only: no index, bound or loop limit changes), to show that tests/test_orb_edges_gpu.py sees it:
#     SLAMHIP_TEST_LIB=tools/exp/libslamhip_orbmut1.so python -m pytest -m gpu tests/test_orb_edges_gpu.py tests/test_orb_gpu.py
# Mutant 3 makes the gather of the selection disagree with its radix select, so fewer keys than the quota can pass and the
# rest of the selection keeps stale coordinates that the describe kernel follows: run it only on
# test_selection_when_every_candidate_ties_on_R, which fails at a quota (1 or 50 of 144) where at least quota keys still pass.
if [ "${1:-}" = "orb-mutants" ]; then
    python3 - "$SRC/orb.hip" "$TMP" <<'EOF'
import sys
src = open(sys.argv[1]).read()
mutants = {
    1: ("s > c[-1] && s > c[1] &&", "s > c[-1] && s >= c[1] &&"),                      # NMS no longer strict towards the right
    2: ("{~((unsigned long long)c.R ^ (1ull << 63)), c.xy}", "{~((unsigned long long)c.R), c.xy}"),      # no sign flip in the key
    3: ("(a.hi == b.hi && a.lo < b.lo)", "(a.hi == b.hi && a.lo > b.lo)"),               # ties on R ordered backwards
    4: ("(unsigned)(ring[i] < p - th) << i", "(unsigned)(ring[i] <= p - th) << i"),      # darker arc one threshold too far
    5: ("(2ll * x * P.W + w) / (2ll * w)", "(2ll * x * P.W) / (2ll * w)"),               # mask x: floor instead of rint
    6: ("        if (lane < 4) { d_kp[4 * slot + lane] = 0; d_desc[4 * slot + lane] = 0ull; }\n        if (lane == 0) d_resp[slot] = 0;\n", ""),
}
for k, (old, new) in mutants.items():
    assert src.count(old) == 1, f"ORB mutant {k} did not apply: the kernel source changed"
    open(f"{sys.argv[2]}/orb_mut{k}.hip", "w").write(src.replace(old, new))
EOF
    ORB_OBJS=$(ls "$ROOT"/slam-experiments_amd/lib/obj/*.o | grep -v "/orb.o")
    for k in 1 2 3 4 5 6; do
        /opt/rocm/bin/hipcc $FLAGS -x hip -c "$TMP/orb_mut$k.hip" -o "$TMP/orb_mut$k.o"
        /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o "$OUT/libslamhip_orbmut$k.so" "$TMP/orb_mut$k.o" $ORB_OBJS -ldl
    done
    rm -rf "$TMP"
    ls -la "$OUT"/libslamhip_orbmut*.so
    exit 0
fi
# tools/build_exp.sh bow-mutants: seven copies of the library, each with ONE deliberate mistake in a temporary copy of bow.hip
# (comparisons and arithmetic on values only: no index, bound, clamp or loop limit changes), to show that
# tests/test_bow_edges_gpu.py sees it:
#     SLAMHIP_TEST_LIB=tools/exp/libslamhip_bowmut1.so python -m pytest -m gpu tests/test_bow_edges_gpu.py tests/test_bow_gpu.py
# Mutants 2 and 7 leave the scatter of the counting sort with offsets that restart at every tile of 4096 keys, so past one tile
# some slots of the permutation are written twice and others never; the index build and the training read rows through that
# permutation, and an unwritten slot of a fresh allocation is not a row: run them only where the permutation is the test's own
# initialised buffer (-k test_group_keys) or where no key count passes one tile (tests/test_bow_gpu.py).
if [ "${1:-}" = "bow-mutants" ]; then
    python3 - "$SRC/bow.hip" "$TMP" <<'EOF'
import sys
src = open(sys.argv[1]).read()
mutants = {
    1: ("        if (i < B) out_off[i] = carry + ex;\n        carry += total;\n", "        if (i < B) out_off[i] = carry + ex;\n", 1),      # offsets: no running total across tiles of 256 images
    2: ("            run += v[u];\n        }\n        carry += total;\n", "            run += v[u];\n        }\n", 1),                # key scan: none across tiles of 4096 keys
    3: ("                if (s_cnt[j]) {\n", "                if (s_acc[j]) {\n", 1),                                              # query: a hit of score 0 is no hit
    4: ("__ballot(2u * bits[(size_t)g * 256 + b] >= m)", "__ballot(2u * bits[(size_t)g * 256 + b] > m)", 1),                    # majority: an exact half clears the bit
    5: ("if (key < bound && key > best) best = key;", "if (key <= bound && key > best) best = key;", 2),                        # query: the previous maximum is selected again
    6: ("t > 0.0", "t >= 0.0", 2),                                                                                              # vectors: words of weight 0 stay
    7: ("int run = carry + bf_block_excl_scan(sum, s_scan, &total);", "int run = bf_block_excl_scan(sum, s_scan, &total);", 1),    # key scan: as 2, but the total in the last slot stays right
}
for k, (old, new, times) in mutants.items():
    assert src.count(old) == times, f"BoW mutant {k} did not apply: the kernel source changed"
    open(f"{sys.argv[2]}/bow_mut{k}.hip", "w").write(src.replace(old, new))
EOF
    BOW_OBJS=$(ls "$ROOT"/slam-experiments_amd/lib/obj/*.o | grep -v "/bow.o")
    for k in 1 2 3 4 5 6 7; do
        /opt/rocm/bin/hipcc $FLAGS -x hip -c "$TMP/bow_mut$k.hip" -o "$TMP/bow_mut$k.o"
        /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o "$OUT/libslamhip_bowmut$k.so" "$TMP/bow_mut$k.o" $BOW_OBJS -ldl
    done
    rm -rf "$TMP"
    ls -la "$OUT"/libslamhip_bowmut*.so
    exit 0
fi
# tools/build_exp.sh bas-mutants: ten copies of the library, each with ONE deliberate mistake in a temporary copy of
# ba_sparse.hip or of the ba_common.h / ba_sparse_phases.h it includes (strides, skips, a comparison and an index that stays inside its array: no
# mutant can leave an array), to show that tests/test_ba_sparse_edges_gpu.py sees it.  Each is run on the narrowest test
# (profiles/ba_sparse_edges_mutants.log names it):
#     SLAMHIP_TEST_LIB=tools/exp/libslamhip_basmut1.so python -m pytest -m gpu tests/test_ba_sparse_edges_gpu.py -k long-delta5
if [ "${1:-}" = "bas-mutants" ]; then
    python3 - "$SRC" "$TMP" <<'EOF'
import os, sys
src, tmp = sys.argv[1], sys.argv[2]
hip, hdr, phases = open(f"{src}/ba_sparse.hip").read(), open(f"{src}/ba_common.h").read(), open(f"{src}/ba_sparse_phases.h").read()
loop = "for (int i = a0 + (int)threadIdx.x; i < a1; i += BA_THREADS) {"
once = "for (int i = a0 + (int)threadIdx.x; i < a1; i = a1) {"


def nth(text, old, new, n, times):
    assert text.count(old) == times, f"BA mutant did not apply ({old!r}): the kernel source changed"
    parts = text.split(old)
    return old.join(parts[:n + 1]) + new + old.join(parts[n + 1:])


mutants = {
    1: ("phases", lambda s: nth(s, loop, once, 0, 2)),                                            # bas_pose_kernel: one trip of its loop
    2: ("phases", lambda s: nth(s, loop, once, 1, 2)),                                            # bas_cost_kernel: one trip
    3: ("hip", lambda s: nth(s, loop, once, 0, 1)),                                               # bas_diag_kernel: one trip
    4: ("hip", lambda s: nth(s, "p < p1; p += 64)", "p < p1; p += 32)", 0, 1)),                   # edge lanes stride 32: pairs taken twice
    5: ("hdr", lambda s: nth(s, " + sw[2][threadIdx.x]) + sw[3][threadIdx.x];", " + sw[2][threadIdx.x]);", 0, 1)),   # ba_block_sum drops wave 3
    6: ("hip", lambda s: nth(s, "        if (fixed[k]) continue;\n", "", 0, 1)),                  # finish: a fixed pose's diagonal in the maximum
    7: ("hip", lambda s: nth(s, "            if (fixed[k]) {\n", "            if (false) {\n", 0, 1)),   # candidate: fixed poses move and count
    8: ("hip", lambda s: nth(s, "step = (int64_t)gridDim.x * BA_THREADS;", "step = BA_THREADS;", 0, 1)),  # candidate: items taken again by other workgroups
    9: ("hdr", lambda s: nth(s, "if (en > delta) {", "if (en >= delta) {", 0, 1)),                # Huber gate no longer strict
    10: ("hip", lambda s: nth(s, "const int n = a * 6 - a * (a - 1) / 2 + (d - a);", "const int n = a * 6 - a * (a + 1) / 2 + (d - a);", 0, 1)),  # Hdiag from a wrong (in-range) packed index
}
for k, (which, f) in mutants.items():
    os.makedirs(f"{tmp}/bas{k}")                       # ba_sparse.hip includes "ba_common.h": the copy beside it wins
    open(f"{tmp}/bas{k}/ba_sparse.hip", "w").write(f(hip) if which == "hip" else hip)
    open(f"{tmp}/bas{k}/ba_common.h", "w").write(f(hdr) if which == "hdr" else hdr)
    open(f"{tmp}/bas{k}/ba_sparse_phases.h", "w").write(f(phases) if which == "phases" else phases)
EOF
    BAS_OBJS=$(ls "$ROOT"/slam-experiments_amd/lib/obj/*.o | grep -v "/ba_sparse.o")
    for k in 1 2 3 4 5 6 7 8 9 10; do
        /opt/rocm/bin/hipcc $FLAGS -x hip -c "$TMP/bas$k/ba_sparse.hip" -o "$TMP/bas$k.o"
        /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o "$OUT/libslamhip_basmut$k.so" "$TMP/bas$k.o" $BAS_OBJS -ldl
    done
    rm -rf "$TMP"
    ls -la "$OUT"/libslamhip_basmut*.so
    exit 0
fi
# tools/build_exp.sh ctx-mutants: four copies of the library, each with ONE initialisation of a context block dropped or one
# layout mistake, to show that tests/test_ctx_poison_gpu.py sees it.  Each is built only because reading the
# code shows that the stale value is compared, added or or-ed and never used as an index, an address or a loop bound
# (profiles/ctx_poison_mutants.log gives the argument per mutant):
#     SLAMHIP_TEST_LIB=tools/exp/libslamhip_ctxmut1.so python -m pytest -m gpu tests/test_ctx_poison_gpu.py tests/test_proj_match_gpu.py
if [ "${1:-}" = "ctx-mutants" ]; then
    python3 - "$SRC" "$TMP" <<'EOF'
import os, sys
src, tmp = sys.argv[1], sys.argv[2]
mutants = {
    # 1: the claim words of SearchByProjection keep what the workspace held
    1: ("proj_match.hip", "proj_match.hip", "    if (search && own2 > 0) SLAM_HIP(hipMemsetAsync(owner, 0xFF, (size_t)own2 * 4, ctx->stream));\n", ""),
    # 2: the RANSAC keys and model counts of the absolute pose keep what the workspace held
    2: ("pnp.hip", "pnp.hip", "    SLAM_HIP(hipMemsetAsync(ws, 0, (size_t)(key_bytes + (uint64_t)B * 4), ctx->stream));\n", ""),
    # 3: the scalar block of the graph solver (status, n_fixed, done, iters) keeps what the workspace held (SE(3) solver only)
    3: ("pose_graph.hip", "graph_lm.h", "    SLAM_HIP(hipMemsetAsync(G.sc, 0, sizeof(glm_scal), st));\n", ""),
    # 4: a host-side layout mistake in SearchByBoW: the claim words start one aligned block early, inside the distance table
    4: ("bow_match.hip", "bow_match.hip", "    p.o_owner = p.o_dist + (own_tables ? slam_align_up((uint64_t)n1_total * 8) : 0);\n",
        "    p.o_owner = p.o_dist + (own_tables ? slam_align_up((uint64_t)n1_total * 8) - 256 : 0);\n"),
}
for k, (unit, patched, old, new) in mutants.items():
    os.makedirs(f"{tmp}/ctx{k}")
    for name in {unit, patched}:                       # a quoted include finds the copy beside the unit first
        text = open(f"{src}/{name}").read()
        if name == patched:
            assert text.count(old) == 1, f"context mutant {k} did not apply: the source changed"
            text = text.replace(old, new)
        open(f"{tmp}/ctx{k}/{name}", "w").write(text)
    open(f"{tmp}/ctx{k}/unit", "w").write(unit)
EOF
    for k in 1 2 3 4; do
        unit=$(cat "$TMP/ctx$k/unit")
        OTHER=$(ls "$ROOT"/slam-experiments_amd/lib/obj/*.o | grep -v "/${unit%.hip}.o")
        /opt/rocm/bin/hipcc $FLAGS -x hip -c "$TMP/ctx$k/$unit" -o "$TMP/ctx$k.o"
        /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o "$OUT/libslamhip_ctxmut$k.so" "$TMP/ctx$k.o" $OTHER -ldl
    done
    rm -rf "$TMP"
    ls -la "$OUT"/libslamhip_ctxmut*.so
    exit 0
fi
# tools/build_exp.sh covis-mutants: ten copies of the library, each with ONE deliberate mistake in a temporary copy of
# covis.hip, to show what tests/test_covis_edges_gpu.py sees that tests/test_covis_gpu.py does not.  No mutant touches a guard:
# every store of the file stays behind its bound (cv_scatter `pos < n`, cv_emit `j >= s + n`, cv_edges `r >= E`, the point
# field checked against L), so a wrong order or a wrong rank yields wrong values, never an address.  Mutants 1 to 3 leave an
# observation sort of 64-bit keys unsorted, after which the pair count P is arbitrary (it sizes the tables): run them only on
# the tests profiles/covis_edges_mutants.log names, where the mistake is met before P is used or only the pair sort is hit.
if [ "${1:-}" = "covis-mutants" ]; then
    python3 - "$SRC/covis.hip" "$TMP" <<'EOF'
import sys
src = open(sys.argv[1]).read()
mutants = {
    # 1: 64-bit observation keys only past 33 bits: the keys of the 33-bit forms are cut to 32
    1: [("y.o64 = y.obits > 32;", "y.o64 = y.obits > 33;")],
    # 2: the digit of a sort pass from the low word of the key (both readers of the digit, so the ranks stay a permutation)
    2: [("(unsigned)(keys[i] >> shift) & (CV_DIGITS - 1)", "((unsigned)keys[i] >> shift) & (CV_DIGITS - 1)"),
        ("(unsigned)(key >> shift) & (CV_DIGITS - 1)", "((unsigned)key >> shift) & (CV_DIGITS - 1)")],
    # 3: no sixth pass
    3: [("static inline int cv_passes(int bits) { return (bits + CV_DIGIT_BITS - 1) / CV_DIGIT_BITS; }",
         "static inline int cv_passes(int bits) { const int p = (bits + CV_DIGIT_BITS - 1) / CV_DIGIT_BITS; return p > 5 ? 5 : p; }")],
    # 4: cv_scan hands its `total` to the first level only
    4: [("    cv_scan(st, scratch, nb, scratch + slam_align_up((uint64_t)nb, 32), total);", "    cv_scan(st, scratch, nb, scratch + slam_align_up((uint64_t)nb, 32), (T*)nullptr);")],
    # 5: ... to the first two levels only
    5: [("    cv_scan(st, scratch, nb, scratch + slam_align_up((uint64_t)nb, 32), total);",
         "    cv_scan(st, scratch, nb, scratch + slam_align_up((uint64_t)nb, 32), nb > CV_SCAN_TILE ? (T*)nullptr : total);")],
    # 6: cv_scan_add skipped for the inner level of a scan of three
    6: [("static void cv_scan(hipStream_t st, T* d, int64_t n, T* scratch, T* total) {", "static void cv_scan(hipStream_t st, T* d, int64_t n, T* scratch, T* total, int depth = 0) {"),
        ("    cv_scan(st, scratch, nb, scratch + slam_align_up((uint64_t)nb, 32), total);", "    cv_scan(st, scratch, nb, scratch + slam_align_up((uint64_t)nb, 32), total, depth + 1);"),
        ("    cv_scan_add<T><<<(unsigned)nb, CV_THREADS, 0, st>>>(d, n, scratch);", "    if (depth == 0) cv_scan_add<T><<<(unsigned)nb, CV_THREADS, 0, st>>>(d, n, scratch);")],
    # 7: cv_row_start in 32 bits
    7: [("cv_row_start(cv_u64 i, cv_u64 n) { return i * (2 * n - i - 1) / 2; }",
         "cv_row_start(cv_u64 i, cv_u64 n) { return (uint32_t)i * (2 * (uint32_t)n - (uint32_t)i - 1) / 2; }")],
    # 8: the bisection of the row starts stops after ten steps (rows of up to 1 024)
    8: [("    while (ihi - ilo > 1) {\n", "    for (int step = 0; step < 10 && ihi - ilo > 1; ++step) {\n")],
    # 9: cv_rows: the upper end of the bisection one point short
    9: [("    int64_t lo = 0, hi = M;\n", "    int64_t lo = 0, hi = M - 1;\n")],
    # 10: cv_rows: the bisection stops after sixteen steps (65 536 points)
    10: [("    int64_t lo = 0, hi = M;\n    while (hi - lo > 1) {\n", "    int64_t lo = 0, hi = M;\n    for (int step = 0; step < 16 && hi - lo > 1; ++step) {\n")],
}
for k, edits in mutants.items():
    text = src
    for old, new in edits:
        assert text.count(old) == 1, f"covis mutant {k} did not apply: the kernel source changed"
        text = text.replace(old, new)
    open(f"{sys.argv[2]}/covis_mut{k}.hip", "w").write(text)
EOF
    CV_OBJS=$(ls "$ROOT"/slam-experiments_amd/lib/obj/*.o | grep -v "/covis.o")
    for k in 1 2 3 4 5 6 7 8 9 10; do
        /opt/rocm/bin/hipcc $FLAGS -x hip -c "$TMP/covis_mut$k.hip" -o "$TMP/covis_mut$k.o"
        /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o "$OUT/libslamhip_covismut$k.so" "$TMP/covis_mut$k.o" $CV_OBJS -ldl
    done
    rm -rf "$TMP"
    ls -la "$OUT"/libslamhip_covismut*.so
    exit 0
fi
# tools/build_exp.sh camera-remap: libslamhip_camremap.so, the library with two knobs in a temporary copy of camera.hip that
# tools/camera_remap_ab.py sets through the environment between calls (profiles/camera_remap_ab.log):
#     SLAM_EXP_REMAP_WG      the workgroup target of slam_cam_remap_u8 (the product: 4096)
#     SLAM_EXP_REMAP_PAIRED  set: the two taps of a source row come from one 16-bit load where both count and both lie inside
#                            the source (tap by tap elsewhere); the loads stay inside the source rows the byte taps read
if [ "${1:-}" = "camera-remap" ]; then
    python3 - "$SRC/camera.hip" "$TMP/camera_exp.hip" <<'EOF'
import sys
src = open(sys.argv[1]).read()
row = '''typedef unsigned short __attribute__((aligned(1))) cam_u16;
__device__ __forceinline__ int cam_row(const uint8_t* __restrict__ img, int64_t pitch, int Ws, int Hs, int x, int y, int wl, int wr, int wy, int border,
                                       bool* ok) {
    if (wy != 0 && wr != 0 && x >= 0 && x + 1 < Ws && y >= 0 && y < Hs) {
        const unsigned v = *reinterpret_cast<const cam_u16*>(img + (int64_t)y * pitch + x);
        return wy * (wl * (int)(v & 255u) + wr * (int)(v >> 8));
    }
    return cam_tap(img, pitch, Ws, Hs, x, y, wl * wy, border, ok) + cam_tap(img, pitch, Ws, Hs, x + 1, y, wr * wy, border, ok);
}

template <bool PAIRED>
'''
edits = [
    ("__global__ __launch_bounds__(CAM_LANES) void cam_remap_kernel(", row + "__global__ __launch_bounds__(CAM_LANES) void cam_remap_kernel("),
    ("                int sum = cam_tap(img, src_pitch, Ws, Hs, x0, y0, (32 - a) * (32 - c), border, &ok);\n",
     "                int sum = 0;\n"
     "                if (PAIRED) sum = cam_row(img, src_pitch, Ws, Hs, x0, y0, 32 - a, a, 32 - c, border, &ok) + cam_row(img, src_pitch, Ws, Hs, x0, y0 + 1, 32 - a, a, c, border, &ok);\n"
     "                else {\n                sum = cam_tap(img, src_pitch, Ws, Hs, x0, y0, (32 - a) * (32 - c), border, &ok);\n"),
    ("                sum += cam_tap(img, src_pitch, Ws, Hs, x0 + 1, y0 + 1, a * c, border, &ok);\n",
     "                sum += cam_tap(img, src_pitch, Ws, Hs, x0 + 1, y0 + 1, a * c, border, &ok);\n                }\n"),
    ("    const int64_t target = 4096;\n",
     '    const char* exp_wg = getenv("SLAM_EXP_REMAP_WG");\n    const int64_t target = exp_wg && atoll(exp_wg) > 0 ? atoll(exp_wg) : 4096;\n'),
    ("    cam_remap_kernel<<<grid, dim3(64, 4), 0, ctx->stream>>>(d_src, (int)B, (int)Hs, (int)Ws, src_pitch, src_stride, d_map, (int)Hd, (int)Wd, border,\n"
     "                                                           d_dst, dst_pitch, dst_stride, d_mask, words);\n",
     '    if (getenv("SLAM_EXP_REMAP_PAIRED"))\n'
     "        cam_remap_kernel<true><<<grid, dim3(64, 4), 0, ctx->stream>>>(d_src, (int)B, (int)Hs, (int)Ws, src_pitch, src_stride, d_map, (int)Hd, (int)Wd, border, d_dst, dst_pitch, dst_stride, d_mask, words);\n"
     "    else\n"
     "        cam_remap_kernel<false><<<grid, dim3(64, 4), 0, ctx->stream>>>(d_src, (int)B, (int)Hs, (int)Ws, src_pitch, src_stride, d_map, (int)Hd, (int)Wd, border, d_dst, dst_pitch, dst_stride, d_mask, words);\n"),
]
for old, new in edits:
    assert src.count(old) == 1, "camera-remap knobs did not apply: the kernel source changed"
    src = src.replace(old, new)
open(sys.argv[2], "w").write(src)
EOF
    CAM_OBJS=$(ls "$ROOT"/slam-experiments_amd/lib/obj/*.o | grep -v "/camera.o")
    /opt/rocm/bin/hipcc $FLAGS -x hip -c "$TMP/camera_exp.hip" -o "$TMP/camera_exp.o"
    /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o "$OUT/libslamhip_camremap.so" "$TMP/camera_exp.o" $CAM_OBJS -ldl
    rm -rf "$TMP"
    ls -la "$OUT"/libslamhip_camremap.so
    exit 0
fi
OBJS=$(ls "$ROOT"/slam-experiments_amd/lib/obj/*.o | grep -v bf_hamming)

python3 - "$SRC/bf_hamming.hip" "$TMP/bf_trace.hip" "$TMP/bf_keep.hip" "$TMP/bf_count.hip" "$TMP/bf_cycles.hip" <<'EOF'
import sys
src = open(sys.argv[1]).read()
T = '    if (tid == 0 && g_trace) { g_trace[4*(by*(int)gridDim.x+bx)+%d] = wall_clock64(); }\n'
H = ('    if (g_trace) { unsigned hw_, xc_; asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)\\n\\ts_getreg_b32 %1, hwreg(HW_REG_XCC_ID)" : "=s"(hw_), "=s"(xc_));\n'
     '        if (tid == 0) g_trace[4*(int)gridDim.x*(int)gridDim.y + by*(int)gridDim.x+bx] = ((unsigned long long)xc_ << 32) | hw_; }\n')   # where the block runs
s = src.replace('    const bool leader = !QUEUE && by < lead;\n', T % 0 + H + '    const bool leader = !QUEUE && by < lead;\n', 1)
s = s.replace('        int buf = 0;\n', '    ' + T % 1 + '        int buf = 0;\n', 1)
s = s.replace('        bool fresh = true;', T % 1 + '        bool fresh = true;', 1)
s = s.replace('    // ---- epilogue: merge,', T % 2 + '    // ---- epilogue: merge,', 1)
s = s.replace('    if (!s_last) return;\n', T % 3 + '    if (!s_last) return;\n', 1)
s = s.replace('typedef uint32_t u32;', 'typedef uint32_t u32;\n__device__ unsigned long long* g_trace = nullptr;\n'
              'extern "C" __attribute__((visibility("default"))) int slam_exp_set_trace(void* p) '
              '{ return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_trace), &p, sizeof(p)); }', 1)
assert s.count('g_trace[') == 6, "trace hooks did not apply: the kernel source changed"
open(sys.argv[2], 'w').write(s)
old = 'if (!merging) __hip_atomic_store(&st.bound[qi], SLAM_BOUND_IDLE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);'
old2 = 'const unsigned long long v = __hip_atomic_exchange(&st.best[qi], ~0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);'
assert src.count(old) == 1 and src.count(old2) == 1, "keep-bound hooks did not apply: the kernel source changed"
# bound form: the final 2nd-best distance stays in bound[]; merge form: the final pair stays in best[] (folding the same rows
# again changes nothing) - either way the next search of the same inputs starts every block at its final threshold
k = src.replace(old, 'if (!merging) __hip_atomic_store(&st.bound[qi], k2 == SLAM_KEY_NONE ? SLAM_BOUND_IDLE : '
                     '(k2 >> SLAM_KEY_IDX_BITS), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);')
k = k.replace(old2, old2 + ' if (merging) __hip_atomic_store(&st.best[qi], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);')
open(sys.argv[3], 'w').write(k)
g = '    if (__builtin_expect(__ballot((int)m >= 0) != 0ull, 0)) {\n'
r = '            if (U > 1 && __ballot((int)mu >= 0) == 0ull) continue;\n'
assert src.count(g) == 1 and src.count(r) == 1, "count hooks did not apply: the kernel source changed"
c = src.replace(g, g + '        if (g_fire && (threadIdx.x & 63) == 0) atomicAdd(&g_fire[U > 1 ? 0 : 2], 1ull);\n')
c = c.replace(r, r + '            if (g_fire && (threadIdx.x & 63) == 0) atomicAdd(&g_fire[1], 1ull);\n')
c = c.replace('typedef uint32_t u32;', 'typedef uint32_t u32;\n__device__ unsigned long long* g_fire = nullptr;\n'
              'extern "C" __attribute__((visibility("default"))) int slam_exp_set_fire(void* p) '
              '{ return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_fire), &p, sizeof(p)); }', 1)
open(sys.argv[4], 'w').write(c)
# cycle stamps: one asm statement per stamp (s_memtime + s_memrealtime + the wait), wave 0 lane 0 stores both
C = ('    if (g_cyc) { unsigned long long c_, r_; asm volatile("s_memtime %%0\\n\\ts_memrealtime %%1\\n\\ts_waitcnt lgkmcnt(0)" : "=s"(c_), "=s"(r_) :: "memory");\n'
     '        if (tid == 0) { g_cyc[8*(by*(int)gridDim.x+bx)+%d] = c_; g_cyc[8*(by*(int)gridDim.x+bx)+%d] = r_; } }\n')
y = src.replace('    const bool leader = !QUEUE && by < lead;\n', C % (0, 1) + '    const bool leader = !QUEUE && by < lead;\n', 1)
y = y.replace('        int buf = 0;\n', C % (2, 3) + '        int buf = 0;\n', 1)
y = y.replace('        bool fresh = true;', C % (2, 3) + '        bool fresh = true;', 1)
y = y.replace('    // ---- epilogue: merge,', C % (4, 5) + '    // ---- epilogue: merge,', 1)
y = y.replace('    if (!s_last) return;\n', C % (6, 7) + '    if (!s_last) return;\n', 1)
y = y.replace('typedef uint32_t u32;', 'typedef uint32_t u32;\n__device__ unsigned long long* g_cyc = nullptr;\n'
              'extern "C" __attribute__((visibility("default"))) int slam_exp_set_cycles(void* p) '
              '{ return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_cyc), &p, sizeof(p)); }', 1)
assert y.count('g_cyc[') == 10, "cycle hooks did not apply: the kernel source changed"
open(sys.argv[5], 'w').write(y)
EOF
for v in trace keep count cycles; do
    /opt/rocm/bin/hipcc $FLAGS -c "$TMP/bf_$v.hip" -o "$TMP/bf_$v.o"
done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o "$OUT/libslamhip_trace.so" "$TMP/bf_trace.o" $OBJS -ldl
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o "$OUT/libslamhip_keepbound.so" "$TMP/bf_keep.o" $OBJS -ldl
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o "$OUT/libslamhip_count.so" "$TMP/bf_count.o" $OBJS -ldl
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o "$OUT/libslamhip_cycles.so" "$TMP/bf_cycles.o" $OBJS -ldl
rm -rf "$TMP"
ls -la "$OUT"
