/*
 * slamhip.h — C ABI of libslamhip.so, the MI355X (gfx950) drop-in for the one
 * data-parallel hot path of ViV99/slam-experiments.
 *
 * The reference is pure Python; its "FFI" for this path is the call into the
 * cv2 / g2o wheels.  Each entry point below names the reference call site it
 * replaces (file:line in /root/reference):
 *
 *   slam_bf_knn2_u256      cv2.BFMatcher(NORM_HAMMING).match / knnMatch(k=2)
 *                          behind BruteForceFeatureMatcher.match
 *                          (feature_matchers.py:33-39), called from
 *                          Frontend._match_features (frontend.py:181-187)
 *   slam_bf_match_filter   the post-match filter of feature_matchers.py:41-43
 *                          (+ Lowe ratio / crossCheck, OpenCV semantics)
 *   slam_reproj_rj_f64     EdgeProjectionPoseOnly.compute_error /
 *                          linearize_oplus (frontend.py:272-291), driven by
 *                          Frontend._correct_current_pose (frontend.py:298-393)
 *   slam_pose_normal_eq_f64 / slam_pose_optimize_f64
 *                          the g2o graph + LM loop of Frontend._correct_current_pose
 *                          (frontend.py:298-393)
 *   slam_tv_*              cv2.findEssentialMat / recoverPose / triangulatePoints behind
 *                          pose_estimation_2d2d and triangulation (utils.py:10-55)
 *   slam_pnp_*             cv2.solvePnPRansac (P3P); no call site in the reference (nearest:
 *                          Frontend._reinitialize_from_keyframe, frontend.py:223-229)
 *   slam_hg_*              cv2.findHomography / decomposeHomographyMat and the H / E model
 *                          choice: the unwritten branch of pose_estimation_2d2d (utils.py:27-29)
 *   slam_sim3_*            ORB-SLAM's Sim3Solver (Horn three-point RANSAC) and a least-squares refit; no call
 *                          site in the reference (nearest: euroc.py:63-66 compares unaligned translations)
 *   slam_orb_*             cv2.ORB behind OrbFeatureDetector (feature_detectors.py:18-26),
 *                          called from Frontend._detect_features (frontend.py:245)
 *   slam_orb_*dist*        the same call with ORB-SLAM's quadtree keypoint distribution and a second,
 *                          lower FAST threshold for cells without a corner (feature_detectors.py:18-26)
 *   slam_comm_*            no reference counterpart (the reference is single
 *                          process); RCCL all-gather of per-shard top-2 rows
 *
 * Conventions
 *   - every function returns 0 on success or a negative slam_status; the
 *     message of the last failure on the calling thread is slam_last_error().
 *   - no exceptions cross the boundary; no torch / numpy types in signatures.
 *   - pointers named d_* are DEVICE pointers obtained from slam_malloc on the
 *     same context; pointers named h_* are host pointers owned by the caller
 *     and only read/written during the call.
 *   - a slam_ctx owns one HIP device + one HIP stream; calls on one ctx are
 *     stream-ordered, different ctxs are independent.  Any number of threads
 *     may call any entry point on one ctx, host-buffer (*_host) and
 *     device-pointer ones alike.  Calls that use a block the ctx owns (its
 *     workspace, merge state, chunk tables, pinned completion / count block,
 *     filter scratch, staging arena) serialise on the ctx's call lock, held
 *     from taking the block through the last launch and, for calls that
 *     wait, through the read-back of their counts.  Device buffers the caller
 *     owns (d_* arguments) remain the caller's business: two threads that
 *     hand one ctx the same output buffer race on it.
 *   - empty inputs are not errors: N == 0 is a no-op; M == 0 yields idx = -1,
 *     dist = INT32_MAX (OpenCV's "no neighbour").
 */
#ifndef SLAMHIP_H
#define SLAMHIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct slam_ctx slam_ctx;

#define SLAM_API __attribute__((visibility("default")))

enum slam_status {
    SLAM_OK = 0,
    SLAM_ERR_INVALID = -1,   /* bad argument (null pointer, negative size, limit exceeded) */
    SLAM_ERR_HIP = -2,       /* a HIP runtime call failed */
    SLAM_ERR_NO_DEVICE = -3, /* no gfx950 device visible */
    SLAM_ERR_RCCL = -4,      /* RCCL missing or a collective failed */
    SLAM_ERR_STATE = -5,     /* call made in the wrong state (e.g. comm not initialised) */
    SLAM_ERR_BUSY = -6       /* a resource condition, not a caller error: a kernel that needs all its workgroups resident at
                                once (slam_ba_optimize_f64) could not get them - retry, or use the multi-launch form */
};

/* descriptor geometry: 256-bit ORB descriptors, one row = 32 bytes
 * (Frame.get_descriptors -> (n,32) uint8, primitives.py:200-205) */
#define SLAM_DESC_BYTES 32
/* top-2 keys pack (distance << 23 | index): one launch covers at most 2^23
 * train rows; larger train sets are looped by the library */
#define SLAM_MAX_TRAIN_PER_PASS (1 << 23)
#define SLAM_NO_MATCH_IDX (-1)
#define SLAM_NO_MATCH_DIST 2147483647

/* ---- library / context ------------------------------------------------- */
SLAM_API const char* slam_last_error(void);
SLAM_API const char* slam_version(void);
SLAM_API int slam_device_count(int* count);
SLAM_API int slam_ctx_create(int device, slam_ctx** out);
SLAM_API int slam_ctx_destroy(slam_ctx* ctx);
SLAM_API int slam_ctx_device(slam_ctx* ctx, int* device);
SLAM_API int slam_sync(slam_ctx* ctx);
/* current sizes of the ctx's grow-only blocks (for tests): h_bytes[0..count), count <= 6, of {workspace, merge state,
 * pinned completion / count block, staging arena (device), staging arena (pinned host), radius tables}; 0 = not yet taken */
SLAM_API int slam_ctx_block_bytes(slam_ctx* ctx, int64_t* h_bytes, int count);
/* fills one scratch block of the ctx with `byte` (for tests of the state contract, DESIGN.md: no call reads a byte of a
 * block that the same call has not written).  block: index as in slam_ctx_block_bytes; 0 (workspace), 3 (staging arena,
 * device), 4 (staging arena, pinned host) and 5 (radius tables) are filled over their whole current size once the stream has
 * drained, and a block not yet taken is a no-op.  Blocks 1 and 2 hold state that survives between calls (idle pattern:
 * slam_bf_state_dirty) and are refused with SLAM_ERR_INVALID, as is any other index. */
SLAM_API int slam_ctx_block_fill(slam_ctx* ctx, int block, int byte);

/* ---- device memory (caller keeps the pointer, library tracks it) ------- */
SLAM_API int slam_malloc(slam_ctx* ctx, uint64_t bytes, void** d_ptr);
SLAM_API int slam_free(slam_ctx* ctx, void* d_ptr);
SLAM_API int slam_memset(slam_ctx* ctx, void* d_ptr, int value, uint64_t bytes);
SLAM_API int slam_copy(slam_ctx* ctx, void* d_dst, const void* d_src, uint64_t bytes); /* device to device, asynchronous on the ctx stream */
SLAM_API int slam_upload(slam_ctx* ctx, void* d_dst, const void* h_src, uint64_t bytes);
SLAM_API int slam_download(slam_ctx* ctx, void* h_dst, const void* d_src, uint64_t bytes);

/* ---- stream timers (HIP events on the ctx stream) ----------------------- */
SLAM_API int slam_timer_start(slam_ctx* ctx);
SLAM_API int slam_timer_stop(slam_ctx* ctx, float* ms); /* synchronises */
/* when enabled, every slam_bf_knn2_u256 / slam_reproj_rj_f64 brackets its
 * dominant kernel with events; slam_prof_read returns count and total ms */
SLAM_API int slam_prof_enable(slam_ctx* ctx, int on);
SLAM_API int slam_prof_read(slam_ctx* ctx, int64_t* launches, double* total_ms); /* synchronises, then resets */

/* ---- hot path 1: brute-force Hamming top-2 ------------------------------ */
/* For each of N query rows, the two nearest of M train rows under
 * popcount(q xor t), ordered by (distance asc, train index asc) — the order
 * cv2.BFMatcher.knnMatch(k=2) produces.  d_idx/d_dist are int32 [N,2];
 * column 0 is the 1-NN (what feature_matchers.py:39 returns), column 1 the
 * 2-NN; missing neighbours are (-1, INT32_MAX).  train_base is added to
 * every reported index (used by shards). */
SLAM_API int slam_bf_knn2_u256(slam_ctx* ctx, const void* d_query, int64_t N,
                      const void* d_train, int64_t M, int64_t train_base,
                      int32_t* d_idx, int32_t* d_dist);

/* Several INDEPENDENT searches in ONE launch: search i is slam_bf_knn2_u256(d_query, N, d_train, M, train_base, d_idx,
 * d_dist) of the i-th entry, bit for bit.  Frame-sized searches (the reference matches <= 200 x 200 per frame,
 * frontend.py:181-187; BASELINE configs[1] is 4096 x 4096) are bound by launch and drain latency on a half-empty chip,
 * not by their scan: crossCheck's forward and reverse search, or a handful of candidate verifications, fill one grid
 * instead of queueing cold ones.  At most SLAM_BF_BATCH_MAX searches per call, each over at most 2^23 train rows;
 * h_searches is a HOST array (the descriptors travel in the kernel arguments; nothing is uploaded).  N == 0 entries are
 * skipped, M == 0 entries report "no neighbour".  Asynchronous on the ctx stream. */
#define SLAM_BF_BATCH_MAX 32
typedef struct slam_bf_search {
    const void* d_query;
    int64_t N;
    const void* d_train;
    int64_t M;
    int64_t train_base;
    int32_t* d_idx;
    int32_t* d_dist;
} slam_bf_search;
SLAM_API int slam_bf_knn2_batch_u256(slam_ctx* ctx, int64_t B, const slam_bf_search* h_searches);

/* Merge G partial top-2 tables ([G][N][2] idx and dist, already holding
 * global indices) into one, by (dist, idx) order.  Used by train-sharded
 * runs and by passes over train sets larger than 2^23 rows. */
SLAM_API int slam_bf_merge_top2(slam_ctx* ctx, const int32_t* d_idx_parts,
                       const int32_t* d_dist_parts, int64_t G, int64_t N,
                       int32_t* d_idx, int32_t* d_dist);

/* Host-pointer convenience (uploads, runs, downloads; PCIe inclusive). */
SLAM_API int slam_bf_knn2_u256_host(slam_ctx* ctx, const uint8_t* h_query, int64_t N,
                           const uint8_t* h_train, int64_t M,
                           int32_t* h_idx, int32_t* h_dist);

/* Top-k search, k in [1, SLAM_BF_KNN_MAX]: cv2.BFMatcher(NORM_HAMMING).knnMatch(query, train, k) for any k up to 32
 * (keyframe voting against a KeyframeDatabase wants more candidates per descriptor than the top-2 search gives).
 * d_idx/d_dist are int32 [N,K], each row ordered by (distance asc, train index asc); missing neighbours (M < K) are
 * (-1, INT32_MAX); train_base is added to every reported index; train sets beyond 2^23 rows run in passes that are
 * merged.  Argument checks and empty inputs as slam_bf_knn2_u256; K outside [1, 32] is SLAM_ERR_INVALID and launches
 * nothing.  Asynchronous on the ctx stream.  K = 1 and K = 2 run this search too (bit-identical to slam_bf_knn2_u256). */
#define SLAM_BF_KNN_MAX 32
SLAM_API int slam_bf_knn_u256(slam_ctx* ctx, const void* d_query, int64_t N, const void* d_train, int64_t M,
                              int64_t train_base, int K, int32_t* d_idx, int32_t* d_dist);
/* cv2.BFMatcher.knnMatch(k) on host buffers: uploads, searches, downloads, one stream synchronisation. */
SLAM_API int slam_bf_knn_u256_host(slam_ctx* ctx, const uint8_t* h_query, int64_t N, const uint8_t* h_train, int64_t M,
                                   int K, int32_t* h_idx, int32_t* h_dist);
/* cv2.BFMatcher.knnMatch(k) over a train set split in G parts: merge G partial top-k tables ([G][N][K] idx and dist,
 * already holding global indices, each row sorted) into one [N,K] table by (dist, idx). */
SLAM_API int slam_bf_merge_topk(slam_ctx* ctx, const int32_t* d_idx_parts, const int32_t* d_dist_parts, int64_t G,
                                int64_t N, int K, int32_t* d_idx, int32_t* d_dist);
/* The launch plan of slam_bf_knn_u256 (cv2.BFMatcher.knnMatch(k)) for N x M on a device with num_cu CUs, WITHOUT a
 * device.  h_plan int32 [8] = {K of the kernel instantiation (4, 8, 16 or 32), query blocks, chunks (grid.y of a full
 * pass), rows per chunk, blocks per CU counted on, passes, bytes of partial tables, 1 when a merge kernel follows}. */
SLAM_API int slam_bf_topk_plan_describe(int num_cu, int64_t N, int64_t M, int K, int32_t* h_plan);

/* Radius search: cv2.BFMatcher(NORM_HAMMING).radiusMatch(query, train, maxDistance) - for each query EVERY train row with
 * distance <= max_distance (compared as a float, as OpenCV's CPU matcher does: d <= floor(max_distance); NaN and negative
 * radii keep nothing, 256 and beyond keep every row; slam_bf_radius_threshold).  The result is compressed-row: d_offsets
 * int64 [N+1], query q's matches are d_idx / d_dist int32 [d_offsets[q], d_offsets[q+1]), ordered by (distance asc,
 * train index asc); train_base is added to every index.  The call counts, scans and reads the total back into *h_total
 * (synchronous).  If the total fits in capacity it also writes the matches (asynchronous behind the read-back: synchronise
 * the stream before reading them); otherwise d_offsets is still valid, nothing else is written and the call returns 0 with
 * *h_total > capacity, so that the caller can grow its buffers and call again.  No state is kept between calls.  Null
 * pointers (d_idx / d_dist may be null when capacity is 0), negative sizes or train_base + M beyond int32 are
 * SLAM_ERR_INVALID and launch nothing.  N = 0 writes d_offsets = {0}; M = 0 gives N empty lists.  No 2^23 limit on M. */
SLAM_API int slam_bf_radius_u256(slam_ctx* ctx, const void* d_query, int64_t N, const void* d_train, int64_t M,
                                 float max_distance, int64_t train_base, int64_t* d_offsets, int64_t capacity,
                                 int32_t* d_idx, int32_t* d_dist, int64_t* h_total);
/* cv2.BFMatcher.radiusMatch on host buffers (the frame-sized drop-in path): uploads, searches, downloads, one stream
 * synchronisation; the same contract as slam_bf_radius_u256 with h_* host arrays.  Returns when the results are in place. */
SLAM_API int slam_bf_radius_u256_host(slam_ctx* ctx, const uint8_t* h_query, int64_t N, const uint8_t* h_train, int64_t M,
                                      float max_distance, int64_t* h_offsets, int64_t capacity, int32_t* h_idx,
                                      int32_t* h_dist, int64_t* h_total);
/* The threshold th of a radius: a row is kept when distance < th; th = floor(max_distance) + 1 clamped to [0, 257]. */
SLAM_API int slam_bf_radius_threshold(float max_distance);
/* The launch plan of slam_bf_radius_u256 for N x M on a device with num_cu CUs, WITHOUT a device.  h_plan int32 [8] =
 * {query blocks, chunks (grid.y of the count and emit kernels), rows per chunk, blocks per CU counted on, passes (always
 * 1: row indices are not packed into keys), bytes of the chunk count table, entries up to which a list is sorted by one
 * wave (longer ones take the tiled path, in tiles of as many entries), distance bins of the sort}. */
SLAM_API int slam_bf_radius_plan_describe(int num_cu, int64_t N, int64_t M, int32_t* h_plan);

/* Window-constrained top-2: cv2.BFMatcher(NORM_HAMMING).knnMatch(query, train, k, mask=W) for the geometric mask the
 * reference draws around each last-frame feature (get_featured_detection_mask, utils.py:58-73, built by
 * Frontend._detect_features, frontend.py:231-251), applied to the per-frame match of Frontend._match_features
 * (frontend.py:181-187): ORB-SLAM's search by projection.  Train row j is a candidate for query i iff
 * fabsf(qx_i - tx_j) <= r_j && fabsf(qy_i - ty_j) <= r_j, in float32, inclusive (the square of cv2.rectangle(pt - r,
 * pt + r, FILLED)); NaN coordinates or radii and negative radii match nothing, r = +inf puts every row in window (the
 * result then equals slam_bf_knn2_u256's).  d_query_xy float32 [N,2] (the current keypoints), d_train_xy float32 [M,2]
 * (window centres: last positions or predicted projections), d_radius float32 [M] per train row, or NULL and the scalar
 * radius.  d_idx / d_dist int32 [N,k], k in {1,2}: the k nearest in-window train rows ordered by (distance asc, train
 * index asc), missing ones (-1, INT32_MAX); bit-identical whatever the grid, the chunking or the order of the atomics.
 * cells caps the cell grid (0 = the shipped rule: about one cell per train row, at most 1024 x 1024; 1 = one cell, a dense
 * scan).  No N x M work or memory: a cell grid over the train centres, its bins, and the candidate rows of each query's
 * neighbourhood; the workspace is the context's (grow-only, slam_bf_window_plan_describe).  Asynchronous on the ctx stream.
 * M >= 2^23 (the 23-bit row field of the selection keys), N > 2^28, k not in {1,2} and null pointers are SLAM_ERR_INVALID
 * and launch nothing.  N = 0 does nothing; M = 0 gives N rows of (-1, INT32_MAX). */
SLAM_API int slam_bf_window_knn_u256(slam_ctx* ctx, const void* d_query, int64_t N, const void* d_train, int64_t M,
                                     const float* d_query_xy, const float* d_train_xy, const float* d_radius, float radius,
                                     int k, int64_t cells, int32_t* d_idx, int32_t* d_dist);
/* The same on host buffers (the frame-sized drop-in of frontend.py:181-187 with windows): uploads, searches, downloads,
 * one stream synchronisation.  h_radius is float32 [M] or NULL (the scalar radius).  Returns when the results are in place. */
SLAM_API int slam_bf_window_knn_u256_host(slam_ctx* ctx, const uint8_t* h_query, int64_t N, const uint8_t* h_train, int64_t M,
                                          const float* h_query_xy, const float* h_train_xy, const float* h_radius,
                                          float radius, int k, int64_t cells, int32_t* h_idx, int32_t* h_dist);
/* The launch plan of slam_bf_window_knn_u256 for N x M under the cell cap `cells` (0 = shipped rule) on a device with
 * num_cu CUs, WITHOUT a device.  h_plan int64 [10] = {cells per axis at most, cells at most, query tiles at most,
 * queries per work item, candidate rows per work item, blocks of the search kernel (4 waves each), parts of the histogram
 * scan (0: one block), parts of the item scan (0: one block), workspace bytes, cells per query tile side at most}.
 * M >= 2^23 and N > 2^28 are SLAM_ERR_INVALID, as in the search. */
SLAM_API int slam_bf_window_plan_describe(int num_cu, int64_t N, int64_t M, int64_t cells, int64_t* h_plan);

/* Tuning overrides for experiments, per context.  h_knobs is an int32 array of up to SLAM_BF_KNOBS entries (missing
 * entries and a NULL array mean 0 = the shipped choice):
 *   [0] R             queries per lane: 1, 2, 4 or 8 (shipped: 1)
 *   [1] blocks_per_cu grid size target (shipped: 16 while there are no more query blocks than CUs, 32 above; train sets
 *                     below 16384 rows follow the chunk rule of [7] instead)
 *   [2] lead_rows     train rows given to the leader chunks: short chunks at the head of the dispatch order that
 *                     publish exact per-query bounds early (shipped: M/8 up to 8192 for M >= 16384, none below);
 *                     -1 = no leaders
 *   [3] lead_chunk    rows per leader chunk, a multiple of 32 (shipped: about one leader block per CU)
 *   [4] tail          number of linearly shrinking chunks at the end of the grid (shipped: up to 32, none for grids of
 *                     at most two blocks per CU); -1 = none
 *   [5] feed          how train rows reach the lanes at R = 1: 1 = through SGPRs (scalar loads, no LDS), -1 = through an LDS
 *                     tile (shipped: SGPRs whenever the rows are in device memory, and for chunks of at least 512 rows; the
 *                     LDS tile for rows in pinned host memory - the zero-copy frame-sized host calls)
 *   [6] cold          rows a chunk folds in WITHOUT a filter when it starts before anybody has published a bound for its
 *                     queries, a multiple of 16 (shipped: 128, and the whole chunk for train sets below 16384 rows whose
 *                     chunks have at most 384 rows); -1 = none
 *   [7] chunk         rows per uniform chunk for train sets below 16384 rows, a multiple of 32 (shipped: one block per CU
 *                     up to 128 rows a chunk, about 8 sqrt(that) beyond, at most 512)
 *   [8] queue         1 = a queue plan: as many worker blocks per query block as are resident at once, whose waves draw
 *                     the chunks by ticket and keep their top-2 from chunk to chunk; -1 = one block per chunk (the plans
 *                     above).  Shipped: a queue plan for train sets of at least 16384 rows when every query block gets at
 *                     least two and at most 256 workers with at least 1024 rows apiece (four, for train sets beyond 131072 rows) and they fill at least 96 % of
 *                     the resident slots; then [7] forces the rows of a
 *                     uniform chunk, [4] > 0 the shortest chunk at the end of the queue, [4] = -1 no shrinking chunks
 *   [9] merge         how the workers of a queue plan exchange what they know: 1 = by merging their best two rows into the
 *                     per-query slot and reading its 2nd row back (the exact 2nd-best distance of everything folded in so
 *                     far), -1 = through a per-query bound (the minimum of the workers' own 2nd-best distances, as the
 *                     one-block-per-chunk plans do).  Shipped: merging from 12 to 96 workers per query block */
#define SLAM_BF_KNOBS 10
SLAM_API int slam_bf_set_tuning(slam_ctx* ctx, const int32_t* h_knobs, int count);
/* The launch plan slam_bf_knn2_u256 would use for N x M on this context: h_plan int32 [10] =
 * {R, query blocks, uniform chunk rows, chunks, leader rows, leader chunks, shrinking tail chunks, CUs,
 *  feed (1 = train rows through SGPRs, 0 = through an LDS tile), unfiltered rows at a cold chunk start}. */
SLAM_API int slam_bf_plan_info(slam_ctx* ctx, int64_t N, int64_t M, int32_t* h_plan);
/* The same plan WITHOUT a device: a pure function of the CU count, the knobs (as slam_bf_set_tuning; NULL / 0 = shipped)
 * and the shape, so that the planner can be held to its invariants on a host without a GPU.  h_plan int32 [14] =
 * slam_bf_plan_info's ten entries (h_plan[7] = num_cu) + {table-free: the kernel computes its chunk from the block index
 * and no boundary table is uploaded, bound-free: no block reads or writes a bound, workers: worker blocks per query block
 * of a queue plan (knob [8]; 0 = one block per chunk), resident: blocks per CU the planner counts on for that, + 256 when the workers exchange by merging (knob [9])}.  The chunk boundary table (chunks + 1
 * ascending row indices from 0 to M) goes to h_tbl (up to tbl_cap entries; may be NULL) and its length to *tbl_len.
 * rows_on_host: the train rows lie in pinned host memory (frame-sized host calls).  qb_all: the query blocks of all the
 * searches that share the launch (slam_bf_knn2_batch_u256), 0 for a search that has the grid to itself. */
SLAM_API int slam_bf_plan_describe(int num_cu, const int32_t* h_knobs, int count, int64_t N, int64_t M, int64_t qb_all,
                                   int rows_on_host, int32_t* h_plan, int32_t* h_tbl, int64_t tbl_cap, int64_t* tbl_len);
/* Which engine runs the top-2 search (slam_bf_knn2_u256 and the calls built on it) on this context: 0 = auto (the shipped
 * choice), 1 = the VALU popcount kernel always, 2 = the matrix-core kernel (a +-1 FP4 dot product on the MFMA units, same
 * results bit for bit) on 16x16x128 tiles wherever it is eligible, 3 = the matrix-core kernel on 32x32x64 tiles wherever 2
 * would be eligible (same results again; slam_bf_mx_tile_describe says which of the two auto runs).  Eligible: one pass of at most 2^23 train rows in device memory with every
 * slam_bf_set_tuning knob at its shipped value (a forced knob describes a VALU plan); auto runs it on the shapes where it
 * measured faster (slam_bf_mx_plan_describe h_plan[7]).  The batch call, pinned-host frame-sized calls and
 * slam_bf_knn_u256 stay on the VALU kernels. */
SLAM_API int slam_bf_set_engine(slam_ctx* ctx, int engine);
/* The matrix-core plan for N x M on a device with num_cu CUs, WITHOUT a device: h_plan int32 [8] = {query blocks, worker
 * blocks per query block, uniform chunk rows, chunks, shrinking chunks at the end of the queue, train rows per LDS stage,
 * blocks per CU counted on, 1 when engine 0 runs this shape on the matrix cores}.  The chunk boundary table (chunks + 1
 * ascending row indices from 0 to M) goes to h_tbl (up to tbl_cap entries; may be NULL) and its length to *tbl_len. */
SLAM_API int slam_bf_mx_plan_describe(int num_cu, int64_t N, int64_t M, int32_t* h_plan, int32_t* h_tbl, int64_t tbl_cap,
                                      int64_t* tbl_len);
/* Which matrix-core kernel a pass of N x M runs on under engine 0, 2 or 3, WITHOUT a device: *h_tile = 16 (16x16x128 tiles)
 * or 32 (32x32x64 tiles).  Both kernels run the plan of slam_bf_mx_plan_describe.  For engine 0 this is the choice on the
 * shapes that h_plan[7] sends to the matrix cores. */
SLAM_API int slam_bf_mx_tile_describe(int engine, int64_t N, int64_t M, int32_t* h_tile);
/* How the 32x32x64 matrix-core kernel gets its train rows on this context: 0 = auto (the shipped choice), 1 = every query
 * block expands the compact rows it scans, 2 = the train set is expanded once per search into a prepared image (a buffer of
 * the context, 128 bytes per row, rebuilt by every search in stream order in front of it: train buffers may be overwritten
 * in place between searches) and the search copies its stages from there.  Same tables bit for bit.  The setting applies to
 * the passes that kernel runs (slam_bf_mx_tile_describe: 32); every other pass keeps its feed.  Any other value is refused. */
SLAM_API int slam_bf_set_mx_feed(slam_ctx* ctx, int feed);
/* The feed a pass of N x M on the 32x32x64 kernel takes under `feed` (0, 1 or 2), WITHOUT a device: *h_feed = 1 or 2. */
SLAM_API int slam_bf_mx_feed_describe(int feed, int64_t N, int64_t M, int32_t* h_feed);
/* For tests: the current size of the context's image buffer (0 = not yet taken), and the buffer filled with `byte` once the
 * stream has drained (no search reads a byte of the image that the same search has not written). */
SLAM_API int slam_bf_mx_image_bytes(slam_ctx* ctx, int64_t* h_bytes);
SLAM_API int slam_bf_mx_image_fill(slam_ctx* ctx, int byte);
/* Pinned train sets: expand a train set that stays fixed once, not once per search.
 * slam_bf_train_pin registers rows [0, M) at d_train (inside one slam_malloc allocation of this context) as fixed and, where
 * some search of this M would take the prepared image (slam_bf_mx_feed_describe_pinned, or feed 2 forced on the context at the
 * time of the call), builds an image of its own for it on the context's stream, behind whatever filled the rows.  A top-2
 * search (slam_bf_knn2_u256, the select, keep and batch forms) whose d_train and M are EXACTLY those of a registration then reads
 * that image where the pinned rule or a forced feed 2 says image, with no image launch of its own; every other search, on any
 * other pointer or M, sub-ranges of a pinned set included, runs as if nothing were pinned.  Same tables bit for bit.
 * The contract is the caller's: between a pin and its unpin the rows are written only directly in front of a
 * slam_bf_train_refresh (which rebuilds the image in stream order, so searches queued earlier see the old rows and later
 * ones the new); a search between the write and the refresh may see either.  Nothing is cached for a buffer that is not
 * pinned: it may be overwritten in place between searches as before.
 * Pinning a pointer that is pinned already replaces the registration (another M included).  A context holds at most 8
 * registrations; one more is refused with SLAM_ERR_INVALID.  slam_bf_train_unpin drops the registration and frees the image
 * behind a stream synchronisation; refresh and unpin of a pointer that is not pinned are refused.  slam_free of an allocation
 * that a pinned set lies in drops the registration first, so a later allocation at the same address never meets a stale image,
 * and slam_ctx_destroy frees every image. */
SLAM_API int slam_bf_train_pin(slam_ctx* ctx, const void* d_train, int64_t M);
SLAM_API int slam_bf_train_refresh(slam_ctx* ctx, const void* d_train);
SLAM_API int slam_bf_train_unpin(slam_ctx* ctx, const void* d_train);
/* The feed a pass of N x M on the 32x32x64 kernel takes under `feed` (0, 1 or 2) when its train set is pinned, WITHOUT a
 * device: *h_feed = 1 or 2.  Never 1 where slam_bf_mx_feed_describe gives 2. */
SLAM_API int slam_bf_mx_feed_describe_pinned(int feed, int64_t N, int64_t M, int32_t* h_feed);
/* For tests: the launches of the image kernel this context has issued so far (one per search of an unpinned set fed from the
 * image, one per pin or refresh that builds an image), and the registrations it holds. */
SLAM_API int slam_bf_mx_image_launches(slam_ctx* ctx, int64_t* h_count);
SLAM_API int slam_bf_train_pins(slam_ctx* ctx, int64_t* h_count);
/* Restore the matcher's per-context merge state to its idle values.  Every search leaves it clean by itself;
 * call this after a search failed part-way (the library does so on a failed launch).  Stream-ordered. */
SLAM_API int slam_bf_reset_state(slam_ctx* ctx);
/* Diagnostics: waits for the context's stream, then counts the 32-bit words of the merge state that are not at their idle
 * value (*h_words; 0 after every completed search, whatever its plan).  A leftover would corrupt the next search silently,
 * so the tests and tools/stress_state.py assert on this directly. */
SLAM_API int slam_bf_state_dirty(slam_ctx* ctx, int64_t* h_words);

/* slam_bf_knn2_u256 and a selection in ONE launch, for the selections that need no reduction over the queries: the block
 * that decodes a query block's result flags its queries as it writes them.
 *   mode 0: 1-NN of every query that has one (bf.match, feature_matchers.py:39,44)
 *   mode 2: Lowe ratio, kept iff dist0 < param * dist1 (strict; needs 2 neighbours) - BASELINE configs[1]
 * d_keep uint8 [N] (1 = kept); *h_count = rows kept, once the search is done (h_count NULL: asynchronous, no count; with a count and <= 16384 queries the call waits by polling completion words in pinned memory, see slam_bf_match_host, otherwise it synchronises the stream).  Same
 * flags and count as slam_bf_knn2_u256 + slam_bf_match_filter; mode 1 (the min-distance filter) needs the global minimum
 * and stays there.  Train sets of more than 2^23 rows and empty ones run the two steps internally. */
SLAM_API int slam_bf_knn2_select_u256(slam_ctx* ctx, const void* d_query, int64_t N, const void* d_train, int64_t M,
                                      int64_t train_base, int32_t* d_idx, int32_t* d_dist, int mode, double param,
                                      uint8_t* d_keep, int64_t* h_count);

/* Post-match selection on the device (feature_matchers.py:41-43 and the
 * OpenCV knn / ratio semantics).  Input: the [N,2] tables above.
 *   mode 0: 1-NN of every query that has one                 (bf.match, feature_matchers.py:39,44)
 *   mode 1: 1-NN kept iff dist < max(2*min_dist, param)      (feature_matchers.py:42-43, strict <)
 *   mode 2: Lowe ratio: kept iff dist0 < param * dist1       (strict; needs 2 neighbours)
 * d_keep is uint8 [N]; *h_count receives the number kept; *h_min_dist the
 * minimum 1-NN distance over all queries (INT32_MAX if none).  Synchronises. */
SLAM_API int slam_bf_match_filter(slam_ctx* ctx, const int32_t* d_idx, const int32_t* d_dist,
                         int64_t N, int mode, double param,
                         uint8_t* d_keep, int64_t* h_count, int32_t* h_min_dist);

/* crossCheck=True selection (cv2.BFMatcher(normType, crossCheck=True).match; OpenCV 4.x batch_distance.cpp
 * crosscheck branch): given the FORWARD search (every query row's nearest train row, [N,2] tables from
 * slam_bf_knn2_u256(query, train)) and the REVERSE search (every train row's nearest query row, [M,2] idx table
 * from slam_bf_knn2_u256(train as query, query as train)), query q keeps its nearest train row t iff q is also
 * t's nearest query row (mutual nearest neighbours, ties to the lowest index on both sides); all other queries
 * get (-1, INT32_MAX).  d_out_idx / d_out_dist are int32 [N].  Synchronises. */
SLAM_API int slam_bf_cross_check(slam_ctx* ctx, const int32_t* d_fwd_idx, const int32_t* d_fwd_dist, int64_t N,
                        const int32_t* d_rev_idx, int64_t M, int32_t* d_out_idx, int32_t* d_out_dist,
                        int64_t* h_count);

/* Multi-image train sets (cv2.BFMatcher.add([...]) + knnMatch, the loop-closure layout; the reference constructs and
 * queries the matcher at feature_matchers.py:34,39, the collection semantics are OpenCV's): the search runs over the
 * concatenated rows of all images - whose order is (imgIdx, trainIdx), so ties resolve as OpenCV's do - and this turns
 * every reported global train row back into the pair.  d_offsets int32 [images + 1]: first row of each image,
 * ascending, d_offsets[0] = 0, d_offsets[images] = total rows; images <= 8191 and fewer than 2^18 rows per image
 * (OpenCV's imgIdx << 18 encoding).  count entries of d_global_idx (e.g. 2 N for an [N,2] table) -> d_img_idx,
 * d_train_idx; -1 ("no neighbour") stays -1 in both.  Asynchronous on the ctx stream. */
SLAM_API int slam_bf_split_index(slam_ctx* ctx, const int32_t* d_global_idx, int64_t count, const int32_t* d_offsets,
                                 int64_t images, int32_t* d_img_idx, int32_t* d_train_idx);

/* ---- hot path 2: reprojection residual + Jacobians (f64) ---------------- */
/* Per observation o with pose k = d_obs_pose[o], point l = d_obs_point[o]:
 *   p_c = R_k p_l + t_k                      (T * pos3d,  frontend.py:275)
 *   e   = meas_o - (fx X/Z + cx, fy Y/Z + cy)            (frontend.py:275-277)
 *   Zinv = 1/(Z + 1e-18); J_pose = 2x6, rotation columns first
 *                                                        (frontend.py:284-291)
 *   J_point = -dproj/dp_c * R_k (2x3)  — extension, not in the reference
 * d_poses: [K,12] f64 = row-major R (9) then t (3), i.e. the top 3x4 of Tcw
 * flattened as [R|t] rows: (r00 r01 r02 tx r10 r11 r12 ty r20 r21 r22 tz).
 * d_points [L,3], d_meas [O,2], outputs d_e [O,2], d_Jpose [O,12] (row-major
 * 2x6), d_Jpoint [O,6] (row-major 2x3) or NULL to skip it. */
SLAM_API int slam_reproj_rj_f64(slam_ctx* ctx, const double* d_poses, int64_t K,
                       const double* d_points, int64_t L,
                       const int32_t* d_obs_pose, const int32_t* d_obs_point,
                       const double* d_meas, int64_t O,
                       double fx, double fy, double cx, double cy,
                       double* d_e, double* d_Jpose, double* d_Jpoint);

/* d_obs_pose / d_obs_point entries must lie in [0, K) / [0, L).  slam_reproj_rj_f64 and the per-observation stage
 * of slam_ba_reduce_f64 never dereference an index outside that range: the observation is computed from row 0
 * with a NaN measurement (its e / J come out NaN) and a per-context counter is bumped.  slam_index_errors returns
 * how many such observations were met since the last call and clears the counter (synchronises).  The derived
 * tables of slam_ba_reduce_f64 (pt_ptr / pt_obs / ps_ptr / ps_obs / lookup) are the caller's to build correctly. */
SLAM_API int slam_index_errors(slam_ctx* ctx, int64_t* count);

/* Pose-only normal equations for one pose (frontend.py:298-365 inner build):
 * H = sum w J^T J (6x6, row-major), b = sum w J^T e (6), chi2[o] = e.e,
 * w = Huber weight with delta (delta <= 0: w = 1); observations whose
 * d_active[o] == 0 are skipped (g2o "level 1" edges, frontend.py:372-377).
 * d_pose [12] as above; outputs d_H [36], d_b [6], d_chi2 [O] on device. */
SLAM_API int slam_pose_normal_eq_f64(slam_ctx* ctx, const double* d_pose,
                            const double* d_points, const double* d_meas,
                            const uint8_t* d_active, int64_t O,
                            double fx, double fy, double cx, double cy,
                            double huber_delta,
                            double* d_H, double* d_b, double* d_chi2);

/* The whole of Frontend._correct_current_pose (frontend.py:298-393) as one launch: `rounds` outer rounds
 * (reference: 4) of `iterations` LM iterations (reference: 10) on one pose against O fixed points, every
 * round restarting from d_pose_in, edges with chi2 > chi2_threshold (reference: 5.991**2) leaving the
 * optimisation after each round, the Huber kernel (delta; reference: 1.0) dropped after round index 2.
 * Outputs: d_pose_out [12], d_inlier uint8 [O] (1 = chi2 <= threshold at the end), d_chi2 [O],
 * d_stats int32 [2] = {inlier count, accepted LM steps}.  Asynchronous on the ctx stream. */
SLAM_API int slam_pose_optimize_f64(slam_ctx* ctx, const double* d_pose_in, const double* d_points,
                                    const double* d_meas, int64_t O, double fx, double fy, double cx, double cy,
                                    int rounds, int iterations, double chi2_threshold, double huber_delta,
                                    double* d_pose_out, uint8_t* d_inlier, double* d_chi2, int32_t* d_stats);

/* The same for B independent frames in ONE launch (one workgroup per frame): frame b owns the edges
 * [d_offsets[b], d_offsets[b+1]) of the concatenated d_points [O_total,3] / d_meas [O_total,2] (d_offsets int32 [B+1],
 * ascending, d_offsets[0] = 0, d_offsets[B] = O_total; a table that is not ascending or leaves [0, O_total] never
 * causes an access outside the arrays: the frame shrinks to the part inside and slam_index_errors counts it), d_pose_in / d_pose_out [B,12],
 * d_inlier / d_chi2 [O_total], d_stats int32 [B,2].  Use: the keyframes of a window against the fixed map, or several
 * relocalisation candidates; the reference refines one frame at a time (frontend.py:298-393). */
SLAM_API int slam_pose_optimize_batch_f64(slam_ctx* ctx, int64_t B, const double* d_pose_in, const double* d_points,
                                          const double* d_meas, const int32_t* d_offsets, int64_t O_total, double fx,
                                          double fy, double cx, double cy, int rounds, int iterations,
                                          double chi2_threshold, double huber_delta, double* d_pose_out,
                                          uint8_t* d_inlier, double* d_chi2, int32_t* d_stats);

/* ---- stereo and level-weighted edges (stereo_edge.h, pose_stereo.hip, ba_stereo.hip) -------------------------
 * The edge model of ORB-SLAM's EdgeSE3ProjectXYZ / EdgeStereoSE3ProjectXYZ (and their OnlyPose forms) under the pose
 * optimisation and the sparse bundle adjustment.  Observation o of point p under pose T (3x4 row-major, world -> camera),
 * (X, Y, Z) = R p + t, measurement d_meas3 [O,3] = (mu, mv, mr), information s = d_info [O]:
 *   prediction   u^ = (fx X + cx Z) / Z, v^ = (fy Y + cy Z) / Z, ur^ = u^ - bf / Z
 *   residuals    e0 = mu - u^, e1 = mv - v^; mr NaN: a MONOCULAR edge (e2 = 0); otherwise a STEREO edge, e2 = mr - ur^
 *   information  s is the inverse variance (ORB-SLAM: 1 / scale[level]^2), finite and >= 0.  s = 0 switches the edge off:
 *                it adds nothing to any sum, its chi2 is still reported.  A negative or non-finite s is counted by
 *                slam_index_errors and taken as 0.
 *   chi2         s (e0^2 + e1^2 [+ e2^2]).  The Huber kernel acts on this weighted chi2 with the width delta_mono or
 *                delta_stereo by kind: if delta > 0 and sqrt(chi2) > delta then w = delta / sqrt(chi2) and
 *                rho = 2 delta sqrt(chi2) - delta^2, otherwise w = 1 and rho = chi2.  Normal-equation terms take the
 *                factor (w s), formed first.
 *   Jacobians    rows 0 and 1 are those of slam_reproj_rj_f64 / slam_bas_linearize_f64 (Zinv = 1 / (Z + 1e-18), rotation
 *                columns first); row 2, in the update convention T <- Exp([w, v]) T:
 *                jp2 = jp0 - bf Zinv^2 (Y, -X, 0, 0, 0, 1), jq2[c] = jq0[c] - bf Zinv^2 R[2][c]; zero for a monocular edge
 *   inlier       s > 0 and Z > 0 and chi2 <= chi2_mono or chi2_stereo by kind (no kernel in this chi2).  Z > 0 is ORB-SLAM's
 *                isDepthPositive; applying it in the pose optimisation too is a deviation.
 * f64 without contraction, only + - * / sqrt: the host build of stereo_edge.h returns the device's bits.  Every buffer is the
 * caller's; no call here takes the context's call lock or its workspace; all are asynchronous on the context's stream. */

/* Per-edge linearisation over an observation table, the three-row counterpart of slam_reproj_rj_f64: d_e [O,3] (row 2 = 0
 * for a monocular edge), d_Jpose [O,3,6], d_Jpoint [O,3,3], d_chi2 [O], d_w [O] (the Huber weight).  An index outside
 * [0, K) / [0, L) is never dereferenced: all outputs of that observation are NaN and slam_index_errors counts it. */
SLAM_API int slam_reproj_rj_stereo_f64(slam_ctx* ctx, const double* d_poses, int64_t K, const double* d_points, int64_t L,
                                     const int32_t* d_obs_pose, const int32_t* d_obs_point, const double* d_meas3,
                                     const double* d_info, int64_t O, double fx, double fy, double cx, double cy, double bf,
                                     double delta_mono, double delta_stereo, double* d_e, double* d_Jpose, double* d_Jpoint,
                                     double* d_chi2, double* d_w);

/* ORB-SLAM's Optimizer::PoseOptimization for B frames in one launch (one workgroup of 256 threads per frame) under the
 * offsets contract of slam_pose_optimize_batch_f64 (clamped, counted, never a wild access; B = 0 and frames without edges
 * are legal): `rounds` rounds (ORB-SLAM: 4) of `iterations` LM iterations (10), every round restarting from d_pose_in, the
 * active set recomputed after every round from the classification of ALL edges (an edge may come back), the Huber kernel
 * dropped after round index 2.  ORB-SLAM's gates are 5.991 / 7.815, its widths their square roots.  Frames of up to
 * SLAM_POSE_STEREO_STAGE edges are kept in LDS, larger ones run on the global arrays.  Fixed-order sums: two runs give equal
 * bits, a frame gives the same bits alone or in a batch.  Outputs: d_pose_out [B,12], d_inlier u8 [O_total] = the
 * classification at the returned pose, d_chi2 [O_total] the weighted chi2 there, d_stats int32 [B,4] = {inliers, accepted LM
 * steps, stereo inliers, edges with s > 0}.  A frame whose edges all have s = 0 returns d_pose_in and no inlier. */
#define SLAM_POSE_STEREO_STAGE 512
SLAM_API int slam_pose_optimize_stereo_batch_f64(slam_ctx* ctx, int64_t B, const double* d_pose_in, const double* d_points,
                                                 const double* d_meas3, const double* d_info, const int32_t* d_offsets,
                                                 int64_t O_total, double fx, double fy, double cx, double cy, double bf, int rounds,
                                                 int iterations, double chi2_mono, double chi2_stereo, double delta_mono,
                                                 double delta_stereo, double* d_pose_out, uint8_t* d_inlier, double* d_chi2,
                                                 int32_t* d_stats);

/* ---- two-view geometry (f64): utils.py:10-28 (pose_estimation_2d2d) and utils.py:32-55 (triangulation), batched ------------
 * Conventions: points 1 are the reference's source_pts (last frame, trainIdx), points 2 its query_pts (current frame,
 * queryIdx); normalised coordinates x = ((u - cx) / fx, (v - cy) / fy, 1); x2^T E x1 = 0 with E [9] row-major; the
 * recovered pose maps frame 1 to frame 2, X2 = R X1 + t, |t| = 1, as [12] row-major 3x4 like d_pose above.  PARITY
 * UNPINNED against OpenCV (absent here): restated from the algorithms' definitions; OpenCV's own RANSAC draws, its
 * early termination and the sign its SVD gives t are not reproduced.  All calls are asynchronous on the ctx stream. */

/* The five-point minimal solver on its own (what cv2.findEssentialMat runs per RANSAC sample, utils.py:24): for each of
 * S samples all real essential matrices through five correspondences d_x1 / d_x2 [S,5,2] (normalised).  d_E [S,10,9]:
 * each with Frobenius norm 1, in ascending order of the root variable (the coefficient of the third null-space vector
 * in the solver's own basis), unused slots zero; d_nroots int32 [S] (0..10).  Whatever the sample (repeated or collinear
 * points, a pure rotation, NaN / inf / 1e150 coordinates) every returned matrix is finite with norm 1 and a sample that
 * yields none returns 0 roots; every loop of the solver is bounded, so the time of a call does not depend on the data
 * by more than a small factor (a sample whose elimination meets a pivot below 1e-4 is solved a second time in
 * another basis: a few in a thousand). */
SLAM_API int slam_tv_fivepoint_f64(slam_ctx* ctx, int64_t S, const double* d_x1, const double* d_x2, double* d_E,
                                   int32_t* d_nroots);

/* cv2.findEssentialMat(source_pts, query_pts, cameraMatrix=K) (utils.py:24) for B frame pairs in one call.  Pair b owns
 * the matches [d_offsets[b], d_offsets[b+1]) of d_px1 / d_px2 [M,2] (pixels; 16-byte aligned); d_offsets int32 [B+1]
 * under the contract of slam_pose_optimize_batch_f64 (a table that is not ascending or leaves [0, M] never causes an
 * access outside the arrays: the pair shrinks to the part inside and slam_index_errors counts it).  B <= 65535.
 * Per pair: H hypotheses (1 <= H <= 2^20), no early termination.  Hypothesis h draws five DISTINCT match indices of the
 * pair's n matches from a counter-based generator, all arithmetic in uint64 (wrapping):
 *     splitmix(x):  x += 0x9E3779B97F4A7C15; x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9;
 *                   x = (x ^ (x >> 27)) * 0x94D049BB133111EB; return x ^ (x >> 31)
 *     word(seed, h, d) = splitmix(splitmix(seed ^ (h * 0xD1B54A32D192ED03)) ^ (d * 0x8CB92BA72F3D8DD7))
 *     index(d) = ((word(seed, h, d) >> 32) * n) >> 32
 *   with the draw number d = 0, 1, 2, ...: an index already drawn is skipped and the next d is taken, until there are
 *   five, in that order.  The pair index b is NOT mixed in: a pair's draws, and so its result, are the same wherever
 *   in whatever batch it stands.
 * Every root of every hypothesis is scored on all n matches by the squared Sampson distance in normalised coordinates,
 * evaluated without fused multiply-adds in exactly this order (x1 = (a, b), x2 = (c, d), E row-major e0..e8):
 *     l0 = e0*a + e1*b + e2;  l1 = e3*a + e4*b + e5;  l2 = e6*a + e7*b + e8;      (E x1)
 *     m0 = e0*c + e3*d + e6;  m1 = e1*c + e4*d + e7;                               (E^T x2)
 *     r = c*l0 + d*l1 + l2;   d2 = r*r / (l0*l0 + l1*l1 + m0*m0 + m1*m1)
 *   inlier iff d2 < (threshold_px / ((fx + fy) / 2))^2 (OpenCV's rule).  Winner: most inliers, ties to the lower
 *   hypothesis index, then the lower root index - found with packed integer keys, so the result is bit-identical for
 *   given (matches, intrinsics, H, threshold, seed) whatever B and whatever order the workgroups finish in.
 * Outputs: d_E [B,9] the winner (Frobenius norm 1), d_inlier uint8 [M] its mask (entries outside every pair: 0),
 * d_stats int32 [B,4] = {inlier count, winning hypothesis, winning root, number of (hypothesis, root) models scored}.
 * A pair of fewer than 5 matches (frontend.py:116) yields E = 0, mask 0, stats {0, -1, -1, 0} and is not an error.
 * Non-finite coordinates are data: a match with a NaN / inf coordinate scores NaN and is never an inlier, a hypothesis
 * that drew one yields no model, d_E is always finite (norm 1, or zero with stats {0, -1, -1, models} when no
 * hypothesis gave a model), and one pair's matches never change another pair's result. */
SLAM_API int slam_tv_essential_ransac_f64(slam_ctx* ctx, int64_t B, const int32_t* d_offsets, const double* d_px1,
                                          const double* d_px2, int64_t M, double fx, double fy, double cx, double cy,
                                          int H, double threshold_px, uint64_t seed, double* d_E, uint8_t* d_inlier,
                                          int32_t* d_stats);

/* cv2.recoverPose(E, source_pts, query_pts, cameraMatrix=K) (utils.py:25) for B pairs (offsets as above).  SVD of
 * d_E [B,9] as E = U diag(s1, s2, s3) V^T, s3 the smallest, with det U = det V = +1 (the third columns take the sign
 * that makes it so); R1 = U W V^T, R2 = U W^T V^T, W = [0 1 0; -1 0 0; 0 0 1] (which of the two an SVD calls R1 depends
 * on how it orders the two equal singular vectors, here as in OpenCV); t = the unit left null vector of E with its largest
 * component (first of equals) positive; the matches with d_inlier_in != 0 (null: all) are triangulated (as
 * slam_tv_triangulate_f64, P1 = [I|0], P2 = [R|t]) under the candidates (R1,t), (R2,t), (R1,-t), (R2,-t); a point is
 * good if its depth is in (0, distance_thresh) in both cameras (OpenCV: 50); most good points win, ties to the lower
 * candidate.  d_pose [B,12], d_inlier_out uint8 [M] (good under the winner; outside every pair: 0), d_stats int32 [B,2]
 * = {good count, candidate}.  E = 0 (no model) gives the identity pose, mask 0, stats {0, -1}; so does any E whose
 * sum of squares is not a positive finite double (a NaN entry; entries near 1e-200 or 1e+200, whose squares under- or
 * overflow).  Any other 3x3 input, essential or not (rank 1, rank 3, unequal singular values), gives a finite pose
 * with R orthonormal, det R = +1 and |t| = 1.  No good point under any candidate: candidate 0, count 0. */
SLAM_API int slam_tv_recover_pose_f64(slam_ctx* ctx, int64_t B, const int32_t* d_offsets, const double* d_px1,
                                      const double* d_px2, int64_t M, double fx, double fy, double cx, double cy,
                                      const double* d_E, const uint8_t* d_inlier_in, double distance_thresh,
                                      double* d_pose, uint8_t* d_inlier_out, int32_t* d_stats);

/* cv2.triangulatePoints as utils.py:49-53 uses it: per point the 4x4 DLT matrix (x P[2] - P[0], y P[2] - P[1] for both
 * views; d_P1 / d_P2 [12] row-major 3x4, d_x1 / d_x2 [N,2] in the coordinates the projections expect, 16-byte aligned),
 * v = its right singular vector of the smallest singular value (eigenvector of A^T A by cyclic Jacobi), |v| = 1,
 * v[3] >= 0; d_X [N,3] = v[:3] / v[3] (utils.py:52-53) and d_w [N] = v[3], so a caller can see points at infinity:
 * for finite input d_w is finite and in [0, 1]; parallel rays give d_w near 0 and a d_X that is huge or infinite, identical
 * cameras (a two-dimensional null space) some unit vector of it. */
SLAM_API int slam_tv_triangulate_f64(slam_ctx* ctx, int64_t N, const double* d_P1, const double* d_P2,
                                     const double* d_x1, const double* d_x2, double* d_X, double* d_w);

/* ---- absolute pose (f64): cv2.solvePnPRansac (SOLVEPNP_P3P), batched ---------------------------------------------------
 * A camera pose from 2D-3D correspondences, for B candidates per call.  The reference has NO call site: the nearest is
 * Frontend._reinitialize_from_keyframe (frontend.py:223-229), which drops the map because it has no such estimate.  Uses:
 * relocalisation candidates, and loop edges with a metric translation (a two-view translation has unit length).
 * Conventions: world points X [M,3], pixels px [M,2], normalised x = ((u - cx) / fx, (v - cy) / fy); the pose is [12]
 * row-major 3x4 like d_pose above with X_cam = R X + t.  PARITY UNPINNED against OpenCV (absent here): restated from the
 * algorithm's definition; OpenCV's own RANSAC draws, its early termination and its final refit are not reproduced.
 * All calls are asynchronous on the ctx stream; workspace comes from the ctx block, nothing is allocated per call. */

/* The P3P minimal solver on its own: for each of S samples every pose that sees the three world points d_X [S,3,3] along
 * the three normalised image points d_x [S,3,2] with all three depths positive.  d_pose [S,4,12]: the 0..4 solutions in
 * ascending order of the solver's root variable (v = depth of point 3 / depth of point 1), unused slots zero;
 * d_nsol int32 [S].  Every returned R is orthonormal with det +1 (to rounding: it is built from two orthonormal frames)
 * and every entry finite.  0 solutions: repeated or collinear world points and repeated image points (sin^2 of the angle
 * below 1e-20), NaN / inf coordinates or coordinates whose squares sum to 1e200 or more (1e150), a world point at the
 * camera centre (its image point is not finite), a quartic whose leading coefficient vanishes.  Every loop of the solver
 * is bounded.  Only + - * / sqrt are used, none of them fused: a host build of the same source gives the same bits. */
SLAM_API int slam_pnp_p3p_f64(slam_ctx* ctx, int64_t S, const double* d_X, const double* d_x, double* d_pose,
                              int32_t* d_nsol);

/* cv2.solvePnPRansac(points, px, K, None, flags=SOLVEPNP_P3P) for B candidates in one call.  Candidate b owns the
 * correspondences [d_offsets[b], d_offsets[b+1]) of d_X [M,3] / d_px [M,2]; d_offsets int32 [B+1] under the contract of
 * slam_pose_optimize_batch_f64 (a table that is not ascending or leaves [0, M] never causes an access outside the
 * arrays: the candidate shrinks to the part inside and slam_index_errors counts it).  B <= 65535.
 * Per candidate: H hypotheses (1 <= H <= 2^20), no early termination.  Hypothesis h draws three DISTINCT indices of the
 * candidate's n correspondences with the generator stated at slam_tv_essential_ransac_f64 (splitmix, word(seed, h, d),
 * index(d) = ((word(seed, h, d) >> 32) * n) >> 32, d = 0, 1, 2, ...: an index already drawn is skipped, until there are
 * three, in that order).  The candidate index b is NOT mixed in.
 * Every solution of every hypothesis is scored on all n correspondences, evaluated without fused multiply-adds in
 * exactly this order (pose row-major p0..p11, point (X, Y, Z), pixel (u, v)):
 *     xc = ((p0*X + p1*Y) + p2*Z) + p3;   yc = ((p4*X + p5*Y) + p6*Z) + p7;   zc = ((p8*X + p9*Y) + p10*Z) + p11;
 *     du = (fx * (xc / zc) + cx) - u;     dv = (fy * (yc / zc) + cy) - v;
 *   inlier iff zc > 0 and du*du + dv*dv < threshold_px * threshold_px (OpenCV's reprojectionError, default 8).
 *   Winner: most inliers, ties to the lower hypothesis index, then the lower solution index - found with packed integer
 *   keys, so the result is bit-identical for given (correspondences, intrinsics, H, threshold, seed) whatever B and
 *   whatever order the workgroups finish in.  The winning hypothesis is solved again when the result is written.
 * Outputs: d_pose [B,12] the winner, d_inlier uint8 [M] its mask (entries outside every candidate: 0), d_stats int32
 * [B,4] = {inlier count, winning hypothesis, winning solution, number of (hypothesis, solution) models scored}.
 * A candidate of fewer than 3 correspondences yields the identity pose, mask 0, stats {0, -1, -1, 0} and is not an
 * error; so does one where no hypothesis gives a model.  Non-finite coordinates are data: a correspondence with a NaN /
 * inf coordinate is never an inlier, a hypothesis that drew one yields no model, d_pose is always finite, and one
 * candidate's data never changes another candidate's result. */
SLAM_API int slam_pnp_ransac_f64(slam_ctx* ctx, int64_t B, const int32_t* d_offsets, const double* d_X,
                                 const double* d_px, int64_t M, double fx, double fy, double cx, double cy, int H,
                                 double threshold_px, uint64_t seed, double* d_pose, uint8_t* d_inlier,
                                 int32_t* d_stats);

/* ---- homography (f64): the unwritten branch of pose_estimation_2d2d (utils.py:27-29), batched ---------------------------
 * utils.py:27-29 raises NotImplementedError above a commented-out cv2.findHomography(source_pts, query_pts, method=RANSAC,
 * ransacReprojThreshold=3).  Conventions as the two-view section: points 1 = source_pts, points 2 = query_pts, H [9]
 * row-major h0..h8 with p2 ~ H p1 in PIXELS, poses [12] row-major 3x4 with X2 = R X1 + t, |t| = 1, plane normals n in
 * frame 1 (n . X1 = d > 0 on the plane, H ~ K (R + t n^T / d) K^-1).  PARITY UNPINNED against OpenCV (absent here):
 * restated from the algorithms' definitions; OpenCV's own draws, its early termination and its refit on the inliers
 * (Levenberg-Marquardt) are not reproduced.  Only + - * / sqrt are used, none of them fused: a host build of the same
 * source gives the same bits.  All calls are asynchronous on the ctx stream; workspace comes from the ctx block, nothing
 * is allocated per call. */

/* The four-point minimal solver on its own (what cv2.findHomography runs per RANSAC sample): d_p1 / d_p2 [S,4,2] in any
 * units (pixels are fine: the points are Hartley-normalised inside), d_H [S,9] with p2 ~ H p1, Frobenius norm 1, the sign
 * that makes the projective weights h6 x + h7 y + h8 of all four sample points positive; d_ok int32 [S].  The null
 * vector of the 8x9 system is taken in closed form by cofactors (four points in general position are a projective
 * basis: with p_i, q_i the normalised homogeneous points, the one opposite the largest triangle taken as the fourth, l = adj([p0 p1 p2]) p3, m = adj([q0 q1 q2]) q3, both from
 * coordinate differences, H_n = sum over cyclic (i,j,k) of (m_i l_j l_k) q_i (p_j x p_k)^T), so no entry of H is assumed
 * non-zero and there is no elimination order.  No model (ok = 0, H = 0): any three of the four points collinear or
 * repeated in either image (sin^2 of an angle of the triangle below 1e-20); a triple with opposite orientation in the
 * two images (OpenCV's subset check); a NaN / inf coordinate or squared coordinates that sum to 1e200 or more (1e150).
 * Every returned H is finite. */
SLAM_API int slam_hg_fourpoint_f64(slam_ctx* ctx, int64_t S, const double* d_p1, const double* d_p2, double* d_H,
                                   int32_t* d_ok);

/* cv2.findHomography(source_pts, query_pts, cv2.RANSAC, threshold_px) for B pairs in one call, in pixels, without
 * intrinsics (the reference's branch for camera=None).  Pair b owns the matches [d_offsets[b], d_offsets[b+1]) of
 * d_px1 / d_px2 [M,2]; d_offsets int32 [B+1] under the contract of slam_pose_optimize_batch_f64 (a table that is not
 * ascending or leaves [0, M] never causes an access outside the arrays: the pair shrinks to the part inside and
 * slam_index_errors counts it).  B <= 65535.  Per pair: H hypotheses (1 <= H <= 2^20), no early termination.
 * Hypothesis h draws four DISTINCT indices of the pair's n matches with the generator stated at
 * slam_tv_essential_ransac_f64 (splitmix, word(seed, h, d), index(d) = ((word(seed, h, d) >> 32) * n) >> 32,
 * d = 0, 1, 2, ...: an index already drawn is skipped, until there are four, in that order).  The pair index b is NOT
 * mixed in.  Every hypothesis with a model is scored on all n matches, without fused operations in exactly this order
 * (point 1 (x, y), point 2 (u, v)):
 *     w = (h6*x + h7*y) + h8;   du = ((h0*x + h1*y) + h2) / w - u;   dv = ((h3*x + h4*y) + h5) / w - v;
 *   inlier iff w > 0 and du*du + dv*dv < threshold_px * threshold_px (OpenCV's one-way transfer error; the reference's
 *   comment has 3).  Winner: most inliers, ties to the lower hypothesis - found with packed integer keys, so the result
 *   is bit-identical for given (matches, H, threshold, seed) whatever B and whatever order the workgroups finish in.  The
 *   winning hypothesis is solved again when the result is written.  There is NO refit on the inliers.
 * Outputs: d_H [B,9] the winner, d_inlier uint8 [M] its mask (entries outside every pair: 0), d_stats int32 [B,4] =
 * {inlier count, winning hypothesis, 0, number of hypotheses that gave a model}.  A pair of fewer than 4 matches yields
 * H = 0, mask 0, stats {0, -1, -1, 0}; one where no hypothesis gave a model H = 0, mask 0, {0, -1, -1, 0}; neither is
 * an error.  Non-finite coordinates are data: such a match is never an inlier, a hypothesis that drew one yields no
 * model, d_H is always finite, and one pair's matches never change another pair's result. */
SLAM_API int slam_hg_ransac_f64(slam_ctx* ctx, int64_t B, const int32_t* d_offsets, const double* d_px1,
                                const double* d_px2, int64_t M, int H, double threshold_px, uint64_t seed, double* d_H,
                                uint8_t* d_inlier, int32_t* d_stats);

/* cv2.decomposeHomographyMat(H, K) and the cheirality vote of cv2.recoverPose, for B pairs (offsets as above; one
 * workgroup per pair).  Hn = K^-1 H K: G = H K by columns (g.0 = fx h.0, g.1 = fy h.1, g.2 = (cx h.0 + cy h.1) + h.2), then
 * rows Hn0 = (G0 - cx G2) / fx, Hn1 = (G1 - cy G2) / fy, Hn2 = G2.  Its singular values s1 >= s2 >= s3 (d_sv [B,3], before
 * any scaling) are the square roots of the eigenvalues of Hn^T Hn by cyclic Jacobi, v1 / v3 the eigenvectors of s1 / s3,
 * each with its largest-magnitude component (first of equals) positive, v2 = v3 x v1.  Hs = +-Hn / s2, the sign for which
 * x2^T Hs x1 > 0 holds for more of the matches with d_inlier_in != 0 (null: all) than x2^T Hs x1 < 0 (a tie: +).
 * Candidates (Ma, Soatto, Kosecka, Sastry): with a = sqrt(1 - (s3/s2)^2), b = sqrt((s1/s2)^2 - 1), ua = unit(a v1 + b v3),
 * ub = unit(a v1 - b v3); per u: n = v2 x u, w1 = unit(Hs v2), w2 = unit(Hs u - (w1 . Hs u) w1), w3 = w1 x w2,
 * R = w1 v2^T + w2 u^T + w3 n^T (orthonormal, det +1, to rounding), t = unit((Hs - R) n), and (t, n) take the sign that
 * makes the largest-magnitude component of n positive.  Ra is the rotation of ua.  d_pose_all [B,4,12] / d_normal_all
 * [B,4,3] hold (Ra, ta, na), (Ra, -ta, -na), (Rb, tb, nb), (Rb, -tb, -nb).  Each candidate triangulates the selected
 * matches exactly as slam_tv_triangulate_f64 does (P1 = [I|0], P2 = [R|t], normalised coordinates) and counts the points
 * with depth in (0, distance_thresh) in both cameras: d_count int32 [B,4].  Most points win, ties to the lower candidate:
 * d_pose [B,12], d_inlier_out uint8 [M] (good under the winner; outside every pair or not selected: 0), d_stats int32
 * [B,4] = {best count, best candidate, second-best count, number of candidates}: best = second-best is the two-fold
 * ambiguity of a plane seen fronto-parallel, and is reported, not hidden.
 * Rotation only: (s1 - s3) / s2 < 1e-9 (the numpy reference measures 2.4e-16 on a camera turning on the spot and 1.25e-6 on a
 * baseline of 1e-6 depths) returns ONE candidate (R, 0) with n = 0, R = U V^T the nearest rotation of Hs, counts 0, mask 0,
 * stats {0, -2, 0, 1}.  H = 0, a NaN entry, a sum of squares of H or Hn that is not a positive finite double, or an s2
 * that is not one: the identity pose, no candidates (all zero), d_sv = 0, stats {0, -1, 0, 0}. */
SLAM_API int slam_hg_decompose_f64(slam_ctx* ctx, int64_t B, const int32_t* d_offsets, const double* d_px1,
                                   const double* d_px2, int64_t M, double fx, double fy, double cx, double cy,
                                   const double* d_H, const uint8_t* d_inlier_in, double distance_thresh,
                                   double* d_pose_all, double* d_normal_all, int32_t* d_count, double* d_pose,
                                   double* d_sv, uint8_t* d_inlier_out, int32_t* d_stats);

/* The model scores of ORB-SLAM's initialiser (Mur-Artal et al. 2015, IV) for B pairs (offsets as above), every match of
 * the pair, in pixels.  With T(A; x, y -> u, v) = du*du + dv*dv of the transfer stated at slam_hg_ransac_f64 under the
 * matrix A, and s2 = sigma * sigma:
 *   S_H: the terms T(H; p1 -> p2) / s2 and T(A; p2 -> p1) / s2, A the adjugate of H entry by entry
 *        a0 = h4*h8 - h5*h7; a1 = h2*h7 - h1*h8; a2 = h1*h5 - h2*h4; a3 = h5*h6 - h3*h8; a4 = h0*h8 - h2*h6;
 *        a5 = h2*h3 - h0*h5; a6 = h3*h7 - h4*h6; a7 = h1*h6 - h0*h7; a8 = h0*h4 - h1*h3;   gate 5.991;
 *   S_E: F = K^-T E K^-1 (columns of E K^-1: a.0 = e.0 / fx, a.1 = e.1 / fy, a.2 = e.2 - (cx a.0 + cy a.1); rows of F:
 *        F0 = A0 / fx, F1 = A1 / fy, F2 = A2 - (cx F0 + cy F1));  l = F p1: l0 = (f0*x + f1*y) + f2, l1, l2 alike;
 *        m0 = (f0*u + f3*v) + f6, m1 = (f1*u + f4*v) + f7;  r = (u*l0 + v*l1) + l2;  the terms (r*r / (l0*l0 + l1*l1)) / s2
 *        and (r*r / (m0*m0 + m1*m1)) / s2;   gate 3.841.
 * A term c below its gate contributes (int64)((5.991 - c) * 1048576.0), any other (NaN too) nothing; the contributions are
 * summed in 64-bit integers, so a sum is exact and independent of the order in which lanes finish.  d_score int64 [B,2] =
 * {S_H, S_E}; d_ratio [B] = (double)S_H / (double)(S_H + S_E), 0 if both are 0.  H = 0 or E = 0 scores 0. */
SLAM_API int slam_hg_model_score_f64(slam_ctx* ctx, int64_t B, const int32_t* d_offsets, const double* d_px1,
                                     const double* d_px2, int64_t M, double fx, double fy, double cx, double cy,
                                     const double* d_H, const double* d_E, double sigma, int64_t* d_score,
                                     double* d_ratio);

/* ---- Sim(3) alignment of map points (f64): ORB-SLAM's Sim3Solver and a least-squares refit, batched ----------------------
 * A monocular map drifts in scale, so the constraint between two keyframes that each hold their own copy of the same map
 * points is a similarity.  The reference has NO call site: it closes no loops, and its driver compares the estimated
 * translation with the ground truth without any alignment (euroc.py:63-66).  Conventions: the two copies of the matched
 * map points are d_X1 / d_X2 [M,3], each in its own camera frame; a model is [13]: the row-major 3x4 [R | t] (like d_pose
 * above) followed by s, and means X2 = s R X1 + t with R orthonormal, det R = +1, s > 0.  R is the rotation of the unit
 * quaternion that is the eigenvector of the largest eigenvalue of Horn's symmetric 4x4 matrix (Horn 1987), found by cyclic
 * Jacobi with a fixed number of sweeps; s = trace(R^T M) / sum |x1 - c1|^2 with M = sum (x2 - c2)(x1 - c1)^T (Umeyama's
 * least-squares scale); t = c2 - s R c1.  A quaternion cannot express a reflection: mirror-image point sets get the best
 * proper rotation.  PARITY UNPINNED against ORB-SLAM's Sim3Solver and OpenCV (both absent here): restated from the
 * algorithm's definition; Sim3Solver's own draws, its early termination and its per-octave sigma table are not reproduced
 * (d_sigma2 is where a caller puts the latter).  Only + - * / sqrt are used, none of them fused: a host build of the same
 * source gives the same bits.  All calls are asynchronous on the ctx stream; workspace comes from the ctx block, nothing
 * is allocated per call. */

/* The three-point minimal solver on its own: d_X1 / d_X2 [S,3,3] -> d_model [S,13], d_ok int32 [S].  fix_scale != 0 forces
 * s = 1 (ORB-SLAM's mbFixScale: stereo / RGB-D).  No model (ok = 0, the identity with s = 1): a repeated or collinear
 * triple in either set (sin^2 of an angle of the triangle below 1e-20, the rule of slam_pnp_p3p_f64); NaN / inf
 * coordinates or coordinates whose squares sum to 1e200 or more (1e150); a scale that is not finite and positive. */
SLAM_API int slam_sim3_threepoint_f64(slam_ctx* ctx, int64_t S, const double* d_X1, const double* d_X2, int fix_scale,
                                      double* d_model, int32_t* d_ok);

/* Sim3Solver for B candidates in one call.  Candidate b owns the correspondences [d_offsets[b], d_offsets[b+1]) of d_X1 /
 * d_X2 [M,3]; d_offsets int32 [B+1] under the contract of slam_pose_optimize_batch_f64 (a table that is not ascending or
 * leaves [0, M] never causes an access outside the arrays: the candidate shrinks to the part inside and slam_index_errors
 * counts it).  B <= 65535.  Per candidate: H hypotheses (1 <= H <= 2^20), no early termination.  Hypothesis h draws three
 * DISTINCT indices of the candidate's n correspondences with the generator stated at slam_tv_essential_ransac_f64
 * (splitmix, word(seed, h, d), index(d) = ((word(seed, h, d) >> 32) * n) >> 32, d = 0, 1, 2, ...: an index already drawn
 * is skipped, until there are three, in that order).  The candidate index b is NOT mixed in.
 * Every hypothesis with a model is scored on all n correspondences by ORB-SLAM's rule, in both images, without fused
 * operations in exactly this order.  Per correspondence (X1 = (a0, a1, a2), X2 = (b0, b1, b2); d_sigma2 double [M,2] =
 * the squared keypoint sigmas in image 1 and image 2, NULL = all 1):
 *     u1 = fx * (a0 / a2) + cx;  v1 = fy * (a1 / a2) + cy;  u2 = fx * (b0 / b2) + cx;  v2 = fy * (b1 / b2) + cy;
 *     g1 = chi2_gate * sigma2[i][0];  g2 = chi2_gate * sigma2[i][1];  both 0 unless a2 > 0 and b2 > 0;
 *   per model, A = s R entry by entry (A_k = s * r_k, R row-major r0..r8, t = (t0, t1, t2)):
 *     x = ((A0*a0 + A1*a1) + A2*a2) + t0;  y = ((A3*a0 + A4*a1) + A5*a2) + t1;  z = ((A6*a0 + A7*a1) + A8*a2) + t2;
 *     du2 = (fx * (x / z) + cx) - u2;  dv2 = (fy * (y / z) + cy) - v2;                  (s R X1 + t seen in image 2)
 *     y0 = b0 - t0;  y1 = b1 - t1;  y2 = b2 - t2;
 *     wx = (r0*y0 + r3*y1) + r6*y2;  wy = (r1*y0 + r4*y1) + r7*y2;  wz = (r2*y0 + r5*y1) + r8*y2;
 *     du1 = (fx * (wx / wz) + cx) - u1;  dv1 = (fy * (wy / wz) + cy) - v1;              (R^T (X2 - t) / s seen in image 1:
 *                                         the division by s > 0 changes neither the projection nor the sign of the depth)
 *   inlier iff z > 0 and wz > 0 and du2*du2 + dv2*dv2 < g2 and du1*du1 + dv1*dv1 < g1: all four depths positive and both
 *   squared pixel errors below chi2_gate * sigma2 (ORB-SLAM: 9.210, chi-square of 2 degrees of freedom at 99 %).
 *   Winner: most inliers, ties to the lower hypothesis - found with packed integer keys, so the result is bit-identical for
 *   given (correspondences, sigmas, intrinsics, H, gate, fix_scale, seed) whatever B and whatever order the workgroups finish
 *   in.  The winning hypothesis is solved again when the result is written.  There is no refit here: slam_sim3_refit_f64.
 * Outputs: d_model [B,13] the winner, d_inlier uint8 [M] its mask (entries outside every candidate: 0), d_stats int32
 * [B,4] = {inlier count, winning hypothesis, 0, number of hypotheses that gave a model}.  A candidate of fewer than 3
 * correspondences, or one where no hypothesis gave a model, yields the identity with s = 1, mask 0, stats {0, -1, -1, 0}
 * and is not an error.  Non-finite coordinates are data: such a correspondence is never an inlier, a hypothesis that drew
 * one yields no model, d_model is always finite, and one candidate's data never changes another candidate's result. */
SLAM_API int slam_sim3_ransac_f64(slam_ctx* ctx, int64_t B, const int32_t* d_offsets, const double* d_X1,
                                  const double* d_X2, int64_t M, const double* d_sigma2, double fx, double fy, double cx,
                                  double cy, int H, double chi2_gate, int fix_scale, uint64_t seed, double* d_model,
                                  uint8_t* d_inlier, int32_t* d_stats);

/* The least-squares fit (Horn / Umeyama) over the correspondences of candidate b with d_mask != 0 (uint8 [M]; NULL: all),
 * one workgroup per candidate (offsets as above, counted alike; B <= 2^24): the refit after RANSAC, a direct fit of clean
 * data, the alignment of a trajectory to its ground truth.  The sums are formed in this order, which the result's bits
 * depend on and nothing else (not B, not the order in which workgroups finish; there are no floating-point atomics):
 *   pass 1: lane l of 256 starts from 0 and adds the coordinates of the selected correspondences at the positions l,
 *           l + 256, l + 512, ... of the candidate, ascending (an unselected position adds nothing); the 256 lanes are
 *           combined by the tree "for stride = 128, 64, ..., 1: lane l < stride adds lane l + stride to its own"; the
 *           centroids c1, c2 are lane 0's sums divided by the number of selected correspondences;
 *   pass 2: the same order and tree for p = X1 - c1, q = X2 - c2 (component by component): M_ij += q_i * p_j,
 *           d1 += (p0*p0 + p1*p1) + p2*p2, d2 += (q0*q0 + q1*q1) + q2*q2.
 * Centring before the products is what keeps the digits at coordinates of 1e4 (a one-pass covariance loses them).
 * d_model [B,13], d_stats int32 [B,2] = {points used, ok}.  ok = 0 gives the identity with s = 1: fewer than 3 selected
 * points; selected points that are collinear or repeated in either set - the two largest eigenvalues l1 >= l2 of Horn's
 * matrix differ by 2 (s2 + s3 sign(det M)) in the singular values of M, and l1 - l2 <= 1e-10 * l1 (the second singular
 * value too small against the first: the sine of the rule above, not its square) means the rotation is not determined;
 * NaN / inf among the selected data or sums of squares of 1e200 or more; a scale that is not finite and positive. */
SLAM_API int slam_sim3_refit_f64(slam_ctx* ctx, int64_t B, const int32_t* d_offsets, const double* d_X1,
                                 const double* d_X2, int64_t M, const uint8_t* d_mask, int fix_scale, double* d_model,
                                 int32_t* d_stats);

/* ---- Sim(3) refinement by reprojection error (sim3_opt.hip): ORB-SLAM's Optimizer::OptimizeSim3, batched -------------------
 * The step between the Sim3Solver above and the fusion: a 7-DoF Levenberg-Marquardt refinement of the similarity between two
 * keyframes on the reprojection error of the matched map points in BOTH images against the MEASURED keypoints, with a Huber
 * kernel, a chi-square gate and a second refinement on the survivors; the number of survivors is what a loop is accepted on.
 * The reference has no call site.  PARITY UNPINNED against ORB-SLAM and g2o (both absent here): the chart below is not g2o's
 * Sim3::log / exp, and the map points are constants, not vertices.  f64, only + - * / sqrt, none of them fused: a host build
 * of the same source gives the same bits.  B candidates a call (B <= 65535), one workgroup each; candidate b owns the
 * correspondences [d_offsets[b], d_offsets[b+1]) under the contract of slam_pose_optimize_batch_f64 (clamped, counted by
 * slam_index_errors; the slices of two candidates must not overlap).  The call is asynchronous on the ctx stream and takes
 * no workspace from the ctx block.
 *
 * Inputs per correspondence i: X1 = (a0, a1, a2) and X2 = (b0, b1, b2) of d_X1 / d_X2 [M,3] as above; d_px1 / d_px2 [M,2] the
 * measured keypoints (u1, v1), (u2, v2) in image 1 and image 2 (NOT the projections of the points); d_sigma2 [M,2] = (g1, g2)
 * the squared keypoint sigmas (NULL: all 1).  d_model_in [B,13]: the start, X2 = s R X1 + t (r0..r8 row-major, t0..t2, s).
 *
 * Residuals at a model, in the operation order of the RANSAC score (A_k = s * r_k):
 *     x = ((A0*a0 + A1*a1) + A2*a2) + t0;  y = ((A3*a0 + A4*a1) + A5*a2) + t1;  z = ((A6*a0 + A7*a1) + A8*a2) + t2;   (Y)
 *     e2 = (u2 - (fx * (x / z) + cx), v2 - (fy * (y / z) + cy));
 *     y0 = b0 - t0;  y1 = b1 - t1;  y2 = b2 - t2;
 *     wx = (r0*y0 + r3*y1) + r6*y2;  wy = (r1*y0 + r4*y1) + r7*y2;  wz = (r2*y0 + r5*y1) + r8*y2;                   (W, not / s)
 *     e1 = (u1 - (fx * (wx / wz) + cx), v1 - (fy * (wy / wz) + cy));
 *     c2 = (e2[0]*e2[0] + e2[1]*e2[1]) / g2;  c1 = (e1[0]*e1[0] + e1[1]*e1[1]) / g1.
 *   Each edge k has its own Huber kernel of width delta on q = sqrt(c_k): q <= delta (or delta = 0): w_k = 1, rho_k = c_k;
 *   else w_k = delta / q, rho_k = (2 * delta) * q - delta * delta.  The cost of a model is the sum of rho2 + rho1 over the
 *   active pairs.
 * Chart (tangent order [omega (3), upsilon (3), sigma], a left update): a = omega / 2, n = (a0*a0 + a1*a1) + a2*a2,
 *     R_d = ((1 - n) I + 2 a a^T + 2 [a]x) / (1 + n)     (Cayley: an exact rotation, equal to Exp(omega) to first order),
 *     s_d = (1 + sigma) + (sigma * sigma) / 2             (positive for every sigma, equal to e^sigma to second order),
 *     S <- (s_d * s, R_d R, s_d * (R_d t) + upsilon).
 *   Jacobians at 0: dY = [-[Y]x, I, Y], dW = R^T [[X2]x, -I, -X2], J_k = -Jpi(P) d(P) with Jpi(P) = [[fx / P2, 0,
 *   -(fx * P0) / P2^2], [0, fy / P2, -(fy * P1) / P2^2]], formed as zi = 1 / P2, J[0][c] = -((fx * zi) * d[0][c] - ((fx * P0) *
 *   (zi * zi)) * d[2][c]), J[1][c] likewise with fy, P1, d[1][c]; dW[i][c] = (r_i * G[0][c] + r_(3+i) * G[1][c]) + r_(6+i) * G[2][c]
 *   for G = [[X2]x, -I, -X2]; the update entry by entry: Q = R_d with Q_ii = ((1 - n) + 2 (a_i a_i)) * (1 / (1 + n)), Q_ij =
 *   (2 (a_i a_j) -+ 2 a_k) * (1 / (1 + n)), (R_d R)_ij = (Q_i0 r_0j + Q_i1 r_1j) + Q_i2 r_2j, t_i' = s_d * ((Q_i0 t0 + Q_i1 t1) +
 *   Q_i2 t2) + upsilon_i.  fix_scale != 0: the sigma column of both is zero, the sigma
 *   component of every step is exactly 0 and s comes back bit for bit.
 * Normal equations: H = sum (w_k / g_k) J_k^T J_k (upper triangle, row by row: 28 terms), b = sum (w_k / g_k) J_k^T e_k
 *   (7 terms) and the cost (1 term): per pair edge 2 is added first, then edge 1.
 * Sums: lane l of 256 starts from 0 and adds the active pairs at the positions l, l + 256, l + 512, ... of the candidate,
 *   ascending; within each group of 64 consecutive lanes the tree "for stride = 32, 16, ..., 1: lane l < stride adds lane
 *   l + stride to its own"; the four group sums are combined as (g0 + g1) + (g2 + g3).  No floating-point atomics: the
 *   bits depend on the candidate's data alone, not on B or on the order in which workgroups finish.
 * Levenberg-Marquardt (g2o's schedule), per stage: linearise at the stage's start, lambda = 1e-5 * max(largest diagonal
 *   entry of H, 1e-12), ni = 2.  Each iteration linearises at the current model (the first one uses the stage's) and makes
 *   up to ten trials: solve (H + lambda I) x = -b by LDL^T; candidate = the update of the model by x; its cost F' over the
 *   active pairs; gain = (F - F') / (sum_i x_i * (lambda * x_i - b_i) + 1e-3).  A trial FAILS when a pivot of the LDL^T is
 *   not finite and positive, when the candidate is not finite with s > 0, when F' is not finite, when an active pair has
 *   z <= 0 or wz <= 0 at the candidate, or when gain is not > 0: then lambda *= ni, ni *= 2.  Otherwise the candidate
 *   becomes the model, lambda *= max(1/3, min(1 - (2 gain - 1)^3, 2/3)), ni = 2, and the iteration ends.  Ten failures in
 *   one iteration end the stage (status bit 4).
 * Schedule (ORB-SLAM: th2 = 10, it0 / it_bad / it_clean = 5 / 10 / 5, at least 10 survivors):
 *   1. inactive from the start and never an inlier: a pair with a non-finite coordinate, pixel or sigma, a2 <= 0 or b2 <= 0,
 *      a sigma that is not positive, or z <= 0 or wz <= 0 at the input model;
 *   2. stage 1: it0 iterations with delta = sqrt(th2) on the active pairs;
 *   3. an active pair stays iff c1 <= th2 and c2 <= th2 and z > 0 and wz > 0 at the current model; nBad = how many left;
 *   4. fewer than min_pairs staying: the candidate is REJECTED (status bit 1);
 *   5. stage 2 from the stage-1 model with delta = 0: it_bad iterations if nBad > 0, else it_clean;
 *   6. the rule of 3. again on the pairs that stayed: this is the mask and the count.
 * Outputs: d_model_out [B,13] (a rejected candidate: its input model bit for bit); d_inlier uint8 [M] (0 for a rejected
 * candidate and outside every candidate); d_chi2 [M,2] = (c1, c2) at the output model for every pair that was active at the
 * start, NaN for the others and for every pair of a rejected candidate (entries outside every candidate are not written);
 * d_stats int32 [B,4] = {inliers, accepted steps, nBad, status}.  Finite data whose squares overflow (coordinates of 1e200, a
 * sigma of 1e-300) stay active by rule 1: the sums are then not finite, every trial of the stage fails on its pivots, and the
 * pairs are judged at the model the stage started from.  An input model that is not finite or has s <= 0 is data:
 * status 1 | 2, the identity with s = 1, mask 0, stats {0, 0, 0, 3}.  d_model_out is always finite and one candidate's data
 * never changes another's result.  Candidates of up to SLAM_SIM3_OPT_STAGE pairs are kept in LDS, larger ones run the same
 * code on the global arrays (d_inlier holds their flags meanwhile).  Returns SLAM_ERR_INVALID before any device call for a
 * null pointer (d_sigma2 excepted; the [M,...] arrays only when M > 0), B < 0 or > 65535, M outside [0, 2^28], th2 not positive and finite, an iteration count
 * outside [0, 1000], min_pairs < 1, focal lengths that are not positive or intrinsics that are not finite. */
#define SLAM_SIM3_OPT_STAGE 512
SLAM_API int slam_sim3_optimize_f64(slam_ctx* ctx, int64_t B, const int32_t* d_offsets, const double* d_X1,
                                    const double* d_X2, const double* d_px1, const double* d_px2, int64_t M,
                                    const double* d_sigma2, const double* d_model_in, double fx, double fy, double cx,
                                    double cy, double th2, int it0, int it_bad, int it_clean, int min_pairs,
                                    int fix_scale, double* d_model_out, uint8_t* d_inlier, double* d_chi2,
                                    int32_t* d_stats);

/* ---- Lens distortion (camera.hip, cam_model.h): Frame::UndistortKeyPoints / ComputeImageBounds of ORB-SLAM, and
 * cv2.initUndistortRectifyMap + cv2.remap ------------------------------------------------------------------------------------
 * Every geometric call of this header takes a pinhole camera (fx, fy, cx, cy).  These four bring the pixels of a real lens to
 * that camera: the keypoints after extraction, or the image before it.  PARITY UNPINNED against OpenCV (absent here): the
 * inverse is Newton's method, not OpenCV's five-step fixed-point iteration, and every point carries a status.  f64, no fused
 * operation, + - * / and sqrt only: a host build of cam_model.h gives the device's bits for every model.  atan and tan below
 * are cam_atan and cam_tan of cam_model.h (argument reduction and Taylor series in the four operations, within about 2 ulp of
 * the true value), not the math library's, which differs by a few ulp between the two builds.
 *
 * A camera record is f64 [SLAM_CAM_RECORD = 16]: {fx, fy, cx, cy, model, k[0..7], 0, 0, 0}; the model code is an exact small
 * double.  Records are HOST arrays and are checked before any launch: every value finite, fx, fy > 0, model in {0, 1, 2}.
 *   model 0, pinhole:      no coefficients.
 *   model 1, radtan:       OpenCV / Brown-Conrady, k = (k1, k2, p1, p2, k3).
 *   model 2, equidistant:  Kannala-Brandt with four coefficients, k = (k1, k2, k3, k4) (cv2.fisheye, Kalibr "equidistant").
 * Forward, normalised (x, y) -> raw pixel (u, v), in this operation order:
 *   radtan:       r2 = x*x + y*y;  rad = 1 + r2*(k1 + r2*(k2 + r2*k3));
 *                 xd = (x*rad + ((2*p1)*x)*y) + p2*(r2 + (2*x)*x);  yd = (y*rad + p1*(r2 + (2*y)*y)) + ((2*p2)*x)*y;
 *   equidistant:  r = sqrt(x*x + y*y);  th = atan(r);  t2 = th*th;  thd = th*(1 + t2*(k1 + t2*(k2 + t2*(k3 + t2*k4))));
 *                 s = thd / r (1 when r == 0);  xd = x*s;  yd = y*s;
 *   pinhole:      xd = x;  yd = y;
 *   all:          u = fx*xd + cx;  v = fy*yd + cy.
 * Inverse, raw pixel (u, v) -> normalised (x, y) and the pinhole pixel (fx*x + cx, fy*y + cy):  x0 = (u - cx)/fx, y0 = (v - cy)/fy;
 *   radtan:       from (x, y) = (x0, y0), exactly `iterations` Newton steps on (xd, yd)(x, y) - (x0, y0) = 0, no early exit: with
 *                 dr = k1 + r2*(2*k2 + r2*(3*k3)), c = ((2*x)*y)*dr + ((2*p1)*x + (2*p2)*y),
 *                 a = (rad + ((2*x)*x)*dr) + ((2*p1)*y + (6*p2)*x),  d = (rad + ((2*y)*y)*dr) + ((6*p1)*y + (2*p2)*x),
 *                 det = a*d - c*c,  x -= (d*ex - c*ey)/det,  y -= (a*ey - c*ex)/det   (the Jacobian is symmetric; adjugate);
 *   equidistant:  rd = sqrt(x0*x0 + y0*y0); from th = rd, `iterations` Newton steps on thd(th) - rd = 0 with the derivative
 *                 1 + t2*(3*k1 + t2*(5*k2 + t2*(7*k3 + t2*(9*k4))));  s = tan(th)/rd (1 when rd == 0);  x = x0*s;  y = y0*s;
 *   pinhole:      x = x0;  y = y0.
 * Status per point (uint8), the first that applies:
 *   3  the input is not finite;
 *   2  no pinhole image exists: radtan - the Jacobian is not positive definite (det > 0 and a + d > 0) at an iterate a step
 *      is taken from (the point lies beyond the fold where the model stops being monotonic; det alone is positive again
 *      where both eigenvalues are negative); equidistant - the derivative is not > 0 at an iterate, or th is not in [0, 1.5);
 *   1  not converged: the residual at the result, max(|xd - x0|, |yd - y0|) (equidistant: |thd(th) - rd|, which bounds it),
 *      is above 64 * 2^-52 * max(1, |x0|, |y0|);
 *   0  converged.
 * For a status other than 0 all four outputs of the point are NaN: no caller receives a plausible wrong number.
 *
 * slam_cam_undistort_f64 / slam_cam_distort_f64: B sets of points, set b owning [h_offsets[b], h_offsets[b+1]) of d_px f64 [n,2]
 * (HOST offsets int64 [B+1], ascending from 0, n = h_offsets[B] <= 2^30); C <= SLAM_CAM_MAX cameras h_cameras [C,16]; set b uses
 * camera h_cam_index[b] (HOST int32 [B]; NULL: camera 0).  d_px_out f64 [n,2], d_norm f64 [n,2] or NULL, d_status uint8 [n];
 * nothing outside [0, n) is written; no output may overlap d_px (the calls do not work in place: SLAM_ERR_INVALID).
 * undistort (replaces cv2.undistortPoints(..., P = K)): raw pixels in, pinhole pixels and
 * normalised coordinates out; iterations in [0, SLAM_CAM_ITERATIONS_MAX], 10 is the default of the Python layer.  distort
 * (replaces cv2.projectPoints on unit-depth points): pinhole pixels of the same fx..cy in, raw pixels and DISTORTED normalised
 * coordinates out; status 3 for an input that is not finite, else 0.  One lane per point; the workgroups of a launch are
 * mapped to sets, so the record and the model are uniform.  Asynchronous on the ctx stream, no memory of the context is used.
 *
 * slam_cam_rectify_map (replaces cv2.initUndistortRectifyMap with CV_16SC2-like fixed point): the map of a Wd x Hd destination
 * image of the pinhole camera h_new_K = (fx', fy', cx', cy') turned by h_R (HOST row-major [9], NULL = identity; taken as a
 * rotation, checked for finiteness only) into the raw image of h_camera: d_map int32 [Hd, Wd, 2], 8-byte aligned.  Entry (i, j):
 *   xn = (j - cx')/fx';  yn = (i - cy')/fy';  X = (R0*xn + R3*yn) + R6;  Y = (R1*xn + R4*yn) + R7;  Z = (R2*xn + R5*yn) + R8
 *   (that is R^T (xn, yn, 1));  (u, v) = forward(X/Z, Y/Z);  entry = (rint(32*u), rint(32*v)), ties to even;
 *   the sentinel (INT32_MIN, INT32_MIN) when Z is not > 0 or |32*u| or |32*v| is not < 2^30 (not finite included).
 *
 * slam_cam_remap_u8 (replaces cv2.remap(..., INTER_LINEAR, BORDER_CONSTANT)): B source images u8 [Hs, Ws] at d_src + b*src_stride
 * with rows src_pitch apart, one map [Hd, Wd, 2], B destination images at d_dst + b*dst_stride with rows dst_pitch apart and
 * an optional validity mask d_mask of the destination's shape, pitch and stride.  Integers only; for the entry (U, V):
 *   x0 = U >> 5, a = U & 31, y0 = V >> 5, b = V & 31;  taps (x0,y0), (x0+1,y0), (x0,y0+1), (x0+1,y0+1) with the weights
 *   (32-a)(32-b), a(32-b), (32-a)b, ab;  a tap outside the source reads `border` (0..255);  dst = (sum + 512) >> 10;
 *   mask = 255 when every tap with a non-zero weight lies inside the source, else 0;  a tap of weight 0 is never loaded;
 *   an entry with U or V equal to INT32_MIN gives dst = border, mask = 0.
 * Bytes of the pitch padding and between images are not written.  Source, destination and mask must not overlap
 * (SLAM_ERR_INVALID): a destination pixel reads source pixels that other lanes may already have replaced.  Sides in [1, SLAM_CAM_SIDE_MAX], pitches >= widths, strides
 * >= pitch*(H-1) + W.  Both outputs can be the image and mask blocks of slam_orb_extract_u8 (pitch W, stride H*W,
 * mask_batched = 1).
 *
 * All four return SLAM_ERR_INVALID before any device call for a null pointer (the optional ones excepted; device pointers only
 * when there is something to do), sizes outside the ranges above, and a record, K' or R that fails its check. */
#define SLAM_CAM_RECORD 16
#define SLAM_CAM_MAX 8
#define SLAM_CAM_ITERATIONS_MAX 100
#define SLAM_CAM_SIDE_MAX 32768
SLAM_API int slam_cam_undistort_f64(slam_ctx* ctx, int64_t B, const int64_t* h_offsets, int64_t C, const double* h_cameras,
                                    const int32_t* h_cam_index, int iterations, const double* d_px, double* d_px_out,
                                    double* d_norm, uint8_t* d_status);
SLAM_API int slam_cam_distort_f64(slam_ctx* ctx, int64_t B, const int64_t* h_offsets, int64_t C, const double* h_cameras,
                                  const int32_t* h_cam_index, const double* d_px, double* d_px_out, double* d_norm,
                                  uint8_t* d_status);
SLAM_API int slam_cam_rectify_map(slam_ctx* ctx, const double* h_camera, const double* h_R, const double* h_new_K, int64_t Wd,
                                  int64_t Hd, int32_t* d_map);
SLAM_API int slam_cam_remap_u8(slam_ctx* ctx, const uint8_t* d_src, int64_t B, int64_t Hs, int64_t Ws, int64_t src_pitch,
                               int64_t src_stride, const int32_t* d_map, int64_t Hd, int64_t Wd, int border, uint8_t* d_dst,
                               int64_t dst_pitch, int64_t dst_stride, uint8_t* d_mask);

/* ---- ORB feature extraction (orb.hip): cv2.ORB behind OrbFeatureDetector (feature_detectors.py:18-26), which
 * Frontend._detect_features calls on every frame with a mask (frontend.py:245) -------------------------------------------
 * A batch of B grayscale u8 images [B,H,W] (any W) goes through the integer-exact specification of DESIGN.md 4d: an L-level
 * pyramid resampled from level 0, FAST-9/16 with score and strict 3x3 non-maximum suppression, integer Harris ranking with
 * a per-level quota under the total order (R descending, y ascending, x ascending), a 32-bin intensity-centroid
 * orientation decided by cross-product signs, and 256 steered comparisons on the binomially blurred level.  PARITY
 * UNPINNED against cv2.ORB (absent here, and its learned pattern is not shipped): the result is a pure function of the
 * arguments and equals the numpy restatement of the specification bit for bit.  The host computes the level sizes, the
 * quotas and the steered pattern table once and passes them in, so every party sees the same numbers:
 *   h_level_w / h_level_h  int32 [L], level 0 = (W, H), each level no larger than the one before, all >= 1
 *   h_quota                int32 [L], keypoints kept per level; N_max = their sum (<= SLAM_ORB_MAX_FEATURES)
 *   table                  int8 [32,256,4] = (ax, ay, bx, by) per orientation bin, every coordinate in [-15, 15]
 * Four launches per call, whatever B and L. */
#define SLAM_ORB_MAX_LEVELS 16
#define SLAM_ORB_MAX_SIDE 8192
#define SLAM_ORB_MAX_BATCH 65535
#define SLAM_ORB_MAX_FEATURES 65536      /* the largest quota sum (and B * sum <= 2^28) */
#define SLAM_ORB_TABLE_BYTES 32768

/* Workspace size and layout for slam_orb_extract_u8 (feature_detectors.py:18-26 / frontend.py:245), no device needed.
 * *bytes = the size to allocate.  h_layout (optional) uint64 [4 + 6 L]: {offset of image 0's block, stride between
 * image blocks, offset of the int32 [B,16] candidate counts, offset of the selection scratch}, then per level
 * {level image, blurred level, score map, candidate list (offsets inside an image block), row pitch in bytes of the
 * three planes (a multiple of 4), capacity of the candidate list}.  A candidate is 16 bytes: int64 R, uint32 x | y << 16,
 * uint32 0.  Argument errors as below. */
SLAM_API int slam_orb_workspace(int64_t B, int64_t H, int64_t W, int L, const int32_t* h_level_w, const int32_t* h_level_h,
                                int64_t n_max, uint64_t* bytes, uint64_t* h_layout);

/* OrbFeatureDetector.detect_and_compute (feature_detectors.py:18-26 / frontend.py:245) for B device-resident images.
 * d_mask (optional) u8 [B,H,W] if mask_batched else [H,W], non-zero = allowed (utils.py:58-74); a keypoint is dropped
 * when its level-0 position is masked out.  Outputs, rows ordered by (level, rank): d_count int32 [B]; d_kp int32
 * [B,N_max,4] = (x, y, level, bin) in level coordinates; d_resp int64 [B,N_max] = R; d_desc u8 [B,N_max,32]; slots past
 * the count are zero.  d_workspace: at least slam_orb_workspace bytes, 16-byte aligned like d_table, d_kp, d_resp, d_desc.
 * Asynchronous on the ctx stream.  SLAM_ERR_INVALID, with nothing launched and no output written: null pointers, B outside
 * [0, 65535], H or W outside [1, 8192], L outside [1, 16], level sizes that break the rules above, a negative quota, a
 * quota sum above SLAM_ORB_MAX_FEATURES, fast_threshold outside [1, 254], a workspace that is too small or misaligned.
 * B = 0 is not an error and does nothing. */
SLAM_API int slam_orb_extract_u8(slam_ctx* ctx, const uint8_t* d_images, int64_t B, int64_t H, int64_t W, const uint8_t* d_mask,
                                 int mask_batched, int L, const int32_t* h_level_w, const int32_t* h_level_h,
                                 const int32_t* h_quota, int fast_threshold, const int8_t* d_table, void* d_workspace,
                                 uint64_t workspace_bytes, int32_t* d_count, int32_t* d_kp, int64_t* d_resp, uint8_t* d_desc);

/* The same call on host buffers (feature_detectors.py:18-26 / frontend.py:245): one upload, four launches, one download,
 * one wait; workspace and staging are the context's (the call holds its lock). */
SLAM_API int slam_orb_extract_u8_host(slam_ctx* ctx, const uint8_t* h_images, int64_t B, int64_t H, int64_t W,
                                      const uint8_t* h_mask, int mask_batched, int L, const int32_t* h_level_w,
                                      const int32_t* h_level_h, const int32_t* h_quota, int fast_threshold,
                                      const int8_t* h_table, int32_t* h_count, int32_t* h_kp, int64_t* h_resp, uint8_t* h_desc);

/* Quadtree keypoint distribution with an adaptive FAST threshold (ORB-SLAM's ORBextractor retries a cell at a
 * lower threshold and spreads the survivors with DistributeOctTree): the second selection mode of the extraction above.
 * Workspace size and layout for slam_orb_extract_dist_u8 (feature_detectors.py:18-26 / frontend.py:245), no device needed.
 * It takes the quotas themselves (the node tables are sized by them).  h_layout (optional) uint64 [4 + 10 L]: the 4 + 6 L
 * entries of slam_orb_workspace, then per level {int32 node index per candidate, node table (64 bytes per node), list of the
 * nodes' best candidates (offsets inside an image block), node capacity = roots + quota + 2, or 0 on a level too small for a
 * feature}.  Argument errors as slam_orb_workspace, and a null or out-of-range quota. */
SLAM_API int slam_orb_dist_workspace(int64_t B, int64_t H, int64_t W, int L, const int32_t* h_level_w, const int32_t* h_level_h,
                                     const int32_t* h_quota, uint64_t* bytes, uint64_t* h_layout);

/* OrbFeatureDetector.detect_and_compute (feature_detectors.py:18-26 / frontend.py:245) with the quadtree selection: the
 * arguments, outputs and row order of slam_orb_extract_u8, with two changes.  FAST and the suppression run at
 * fast_threshold_min; a candidate is live if it scores >= fast_threshold or if its 32 x 32 cell ((x-16) >> 5, (y-16) >> 5)
 * holds no candidate that does.  Per level the live candidates are spread over a quadtree whose fullest nodes are split
 * until there are quota[l] of them; every node gives its best candidate under (R descending, y, x) and the best quota[l] of
 * those are kept: min(quota[l], live candidates) rows.  With fast_threshold_min == fast_threshold and a quota above the
 * candidate count the outputs equal those of slam_orb_extract_u8 bit for bit.  The result does not depend on the order in
 * which the candidates were appended.  d_workspace: at least slam_orb_dist_workspace bytes.  Four launches.  Errors as
 * slam_orb_extract_u8, and fast_threshold_min outside [1, fast_threshold]: SLAM_ERR_INVALID, nothing launched, no output
 * written.  B = 0 does nothing.  There is no host-buffer form. */
SLAM_API int slam_orb_extract_dist_u8(slam_ctx* ctx, const uint8_t* d_images, int64_t B, int64_t H, int64_t W, const uint8_t* d_mask,
                                      int mask_batched, int L, const int32_t* h_level_w, const int32_t* h_level_h,
                                      const int32_t* h_quota, int fast_threshold, int fast_threshold_min, const int8_t* d_table,
                                      void* d_workspace, uint64_t workspace_bytes, int32_t* d_count, int32_t* d_kp, int64_t* d_resp,
                                      uint8_t* d_desc);

/* ---- Stereo matching (stereo.hip, stereo_point.h): Frame::ComputeStereoMatches of ORB-SLAM (the reference opens one camera
 * only) -------------------------------------------------------------------------------------------------------------------
 * P pairs of rectified images, h_pairs HOST int32 [P,2] = (image of the left block, image of the right block).  A block is what
 * slam_orb_extract_u8 or slam_orb_extract_dist_u8 left on the device for B images: d_count int32 [B], d_kp int32 [B,N_max,4] =
 * (x, y, level, bin) in level coordinates, d_desc u8 [B,N_max,32] and the extractor's workspace, where the pyramids are.  Both
 * blocks share N_max and one level layout, given as HOST values taken from slam_orb_workspace's layout: image_base and
 * image_stride, and per level h_level_offset uint64 [L] (the level image inside an image block), h_level_pitch, h_level_w,
 * h_level_h int32 [L].  The same block may be passed as left and right.  h_scale HOST f32 [L] = float32(s) ** arange(L) as
 * OrbResult makes it, each in [1, 65536]: no pow runs on the device.  Keypoints must lie inside their level (the extractor's
 * do); a row whose level is outside [0, L) neither has nor is a candidate.  A count is clamped to [0, N_max].
 *
 * The level-0 pixel of a row is the single f32 product (float)x * h_scale[l], promoted to f64; everything below is f64 or
 * integer, unfused, in the order written (tests/stereo_ref.py is the numpy statement).  For a left row i with
 * (uL, vL, lL):
 *   1. a right row j with (uR, vR, lR) is a candidate when floor(vR - r) <= trunc(vL) <= ceil(vR + r) with r = 2 h_scale[lR],
 *      lL - 1 <= lR <= lL + 1, and uL - max_d <= uR <= uL - min_d; a left row with uL - min_d < 0 has none;
 *   2. the candidate of the smallest (Hamming distance, j) is taken, and the row goes on if that distance is < th_orb;
 *   3. on level lL of both pyramids, on the row y = y_level of the left keypoint: left centre x = x_level, right centre
 *      c0 = floor(uR / h_scale[lL] + 0.5).  Status "window" unless c0 - Ls - w >= 0, c0 + Ls + w + 1 < level_w, and the left
 *      patch and the rows y +- w lie inside the level.  For inc in [-Ls, Ls]
 *      SAD(inc) = sum over dy, dx in [-w, w] of |(IL(y+dy, x+dx) - IL(y, x)) - (IR(y+dy, c0+inc+dx) - IR(y, c0+inc))|;
 *      the best is the smallest (SAD, inc); status "slide border" if that inc is -Ls or Ls;
 *   4. d1, d2, d3 = SAD(inc-1), SAD(inc), SAD(inc+1); den = d1 + d3 - 2 d2 (>= 0); delta = 0 if den = 0, else
 *      (double)(d1 - d3) / (double)(2 den), so |delta| <= 1/2;
 *   5. u_right = h_scale[lL] * ((c0 + inc) + delta), disp = uL - u_right; accepted when min_d <= disp < max_d, else status
 *      "disparity"; disp <= 0 becomes disp = 0.01 and u_right = uL - 0.01; depth = bf / disp;
 * and once per pair, if `reject`:
 *   6. with m the SAD at index n / 2 of the n accepted rows in ascending (SAD, i), a row is kept when 10 SAD < 21 m, else its
 *      status is "median" (ORB-SLAM compares with 1.5f * 1.4f * m in float: the two differ at exact equality only).
 * Outputs [P,N_max] each: d_right int32 = the row taken in step 2 (-1: no candidate); d_u_right, d_depth f64 (NaN unless the
 * status is 0); d_orb_dist int32 (256: no candidate); d_sad int32 = the best SAD (-1 for status 1, 2 and 3); d_status u8:
 *   0 matched, 1 no candidate, 2 descriptor distance >= th_orb, 3 window, 4 slide border, 5 disparity out of range,
 *   6 rejected by the median;
 * slots at or past the left image's count are status 1 rows.  d_counts int32 [P,2] = (rows of status 0, rows accepted before
 * step 6).  The result is a pure function of the arguments.  d_workspace: slam_stereo_workspace bytes, 16-byte aligned like
 * d_kp and d_desc; it holds the level table and the pair table.  Two copies and three launches whatever P is, asynchronous on
 * the ctx stream, no memory of the context is used.  SLAM_ERR_INVALID with nothing launched: null pointers (device pointers
 * only when P > 0 and N_max > 0), P outside [0, SLAM_STEREO_MAX_PAIRS], N_max outside [0, SLAM_STEREO_MAX_ROWS], L outside
 * [1, SLAM_STEREO_MAX_LEVELS], a pair outside its block, th_orb outside [0, 256], w or Ls outside [1, SLAM_STEREO_HALF_MAX],
 * bf not positive and finite, min_d not finite, max_d <= min_d (or NaN), a level side outside [1, SLAM_STEREO_MAX_SIDE] or a
 * pitch below its width, a scale outside [1, 65536], a workspace that is too small or misaligned.  P = 0 does nothing. */
#define SLAM_STEREO_MAX_PAIRS 4096
#define SLAM_STEREO_MAX_ROWS 8192
#define SLAM_STEREO_MAX_LEVELS 16
#define SLAM_STEREO_MAX_SIDE 8192
#define SLAM_STEREO_HALF_MAX 15
SLAM_API int slam_stereo_workspace(int64_t P, int64_t n_max, uint64_t* bytes);
SLAM_API int slam_stereo_match(slam_ctx* ctx, int64_t P, const int32_t* h_pairs, int64_t B_left, const int32_t* d_count_left,
                               const int32_t* d_kp_left, const uint8_t* d_desc_left, const void* d_ws_left, int64_t B_right,
                               const int32_t* d_count_right, const int32_t* d_kp_right, const uint8_t* d_desc_right,
                               const void* d_ws_right, int64_t n_max, int L, uint64_t image_base, uint64_t image_stride,
                               const uint64_t* h_level_offset, const int32_t* h_level_pitch, const int32_t* h_level_w,
                               const int32_t* h_level_h, const float* h_scale, double bf, double min_d, double max_d, int th_orb,
                               int w, int Ls, int reject, void* d_workspace, uint64_t workspace_bytes, int32_t* d_right,
                               double* d_u_right, double* d_depth, int32_t* d_orb_dist, int32_t* d_sad, uint8_t* d_status,
                               int32_t* d_counts);

/* ---- per-frame calls on caller-owned host buffers: one upload, one download, one wait (frame-sized: zero-copy, polled) ---- */
/* BruteForceFeatureMatcher.match (feature_matchers.py:36-44; cv2.BFMatcher.match + the min-distance filter) in
 * one call.  Query rows h_query [N,32]; train rows either h_train [M,32] (host) or d_train (device, e.g. the
 * previous frame kept by an earlier call) - exactly one of them when M > 0.  If d_query_keep is non-null the
 * query rows are uploaded there (32*N bytes, caller-allocated with slam_malloc) so the next frame can pass it
 * as d_train.  mode/param as slam_bf_match_filter, plus mode 3 = crossCheck (cv2.BFMatcher(normType,
 * crossCheck=True).match; the reverse search runs in the same call, param unused).  Outputs (caller-allocated, N entries each): the kept
 * matches in ascending query order as query index, train index and distance (float32, integer-valued like
 * cv2's); *h_count = how many.  N == 0 or M == 0: no matches, not an error.
 * Frame-sized calls (<= 4096 rows a side) return as soon as the call's last kernel has stored its completion word into
 * pinned host memory behind its results - the host polls that word instead of synchronising the stream (about 4 us less
 * per call); a call that is not complete after 2 ms of polling waits for the stream as before.  The outputs are complete
 * when the function returns either way. */
SLAM_API int slam_bf_match_host(slam_ctx* ctx, const uint8_t* h_query, int64_t N, const uint8_t* h_train,
                                const void* d_train, int64_t M, void* d_query_keep, int mode, double param,
                                int32_t* h_query_idx, int32_t* h_train_idx, float* h_distance, int64_t* h_count);
/* Bytes the host-buffer entry points (slam_bf_knn2_u256_host, slam_bf_match_host, slam_pose_optimize_host_f64)
 * have moved over PCIe on this context since it was created: inputs copied or read in place by the kernels
 * (h2d), results copied or written in place (d2h).  Rows passed as device pointers (d_train) count nothing. */
SLAM_API int slam_io_counters(slam_ctx* ctx, uint64_t* h2d_bytes, uint64_t* d2h_bytes);
/* slam_pose_optimize_f64 on host buffers (Frontend._correct_current_pose, frontend.py:298-393): h_pose_in [12],
 * h_points [O,3], h_meas [O,2] -> h_pose_out [12], h_inlier uint8 [O], h_chi2 [O], h_stats int32 [2].  Up to 512 edges the
 * kernel reads and writes the pinned staging block itself and the call waits for its completion word (see slam_bf_match_host). */
SLAM_API int slam_pose_optimize_host_f64(slam_ctx* ctx, const double* h_pose_in, const double* h_points,
                                         const double* h_meas, int64_t O, double fx, double fy, double cx,
                                         double cy, int rounds, int iterations, double chi2_threshold,
                                         double huber_delta, double* h_pose_out, uint8_t* h_inlier,
                                         double* h_chi2, int32_t* h_stats);

/* Reduced camera system of a keyframe-window bundle adjustment (extension: the reference's Backend is an
 * empty class, backend.py:101-103; residual/Jacobian arithmetic as frontend.py:272-291).  One call =
 * linearise all O observations, Schur-eliminate the L points with damping `lambda`, and leave on device:
 *   d_rec  [O,SLAM_BA_REC] per-observation blocks (Hpl, Y = Hpl E, ...), d_E [L,9] = (Hll+lambda I)^-1,
 *   d_bl [L,3], d_Hpp [K,21] (upper triangles), d_bp [K,6], d_ybl [K,6] = sum Y bl, d_cost [K] (robust cost
 *   per pose), d_W [K,K,36] with W[k1,k2] = sum_l Y_(k1,l) Hpl_(k2,l)^T for k1 <= k2 (other blocks untouched),
 *   d_hll_diag [L,3] = diagonal of the undamped Hll (optional, may be null; for the initial damping).
 * The caller assembles S = blockdiag(Hpp + lambda I) - W (symmetric), rhs = -bp + ybl, solves for dp [K,6] and
 * calls slam_ba_backsub_f64 for the point updates dl [L,3].
 * Index tables (int32, device): obs_pose/obs_point [O]; pt_ptr [L+1]/pt_obs [O] = observations grouped by
 * point; ps_ptr [K+1]/ps_obs [O] = grouped by pose; lookup [K,L] = observation index of (pose, point) or -1.
 * All reductions run in a fixed order: results are bit-identical from run to run. */
#define SLAM_BA_REC 73
SLAM_API int slam_ba_reduce_f64(slam_ctx* ctx, const double* d_poses, int64_t K, const double* d_points,
                                int64_t L, const int32_t* d_obs_pose, const int32_t* d_obs_point,
                                const double* d_meas, int64_t O, const int32_t* d_pt_ptr, const int32_t* d_pt_obs,
                                const int32_t* d_ps_ptr, const int32_t* d_ps_obs, const int32_t* d_lookup,
                                double fx, double fy, double cx, double cy, double huber_delta, double lambda,
                                double* d_rec, double* d_E, double* d_bl, double* d_Hpp, double* d_bp,
                                double* d_ybl, double* d_cost, double* d_W, double* d_hll_diag);
/* Robust cost of a candidate state only, per pose (d_cost [K]); same tables as slam_ba_reduce_f64. */
SLAM_API int slam_ba_cost_f64(slam_ctx* ctx, const double* d_poses, int64_t K, const double* d_points,
                              const int32_t* d_obs_point, const double* d_meas, const int32_t* d_ps_ptr,
                              const int32_t* d_ps_obs, double fx, double fy, double cx, double cy,
                              double huber_delta, double* d_cost);
SLAM_API int slam_ba_backsub_f64(slam_ctx* ctx, int64_t L, const int32_t* d_pt_ptr, const int32_t* d_pt_obs,
                                 const int32_t* d_obs_pose, const double* d_rec, const double* d_E,
                                 const double* d_bl, const double* d_dp, double* d_dl);

/* A whole window bundle adjustment in ONE launch: Levenberg-Marquardt with Schur complement as a persistent kernel of a
 * few dozen workgroups - the elimination of slam_ba_reduce_f64 as four phases separated by grid barriers (no per-observation
 * records: every phase linearises the observations it touches again), the dense L D L^T solve of the reduced camera system
 * in LDS, the exp() update, the candidate's cost and the accept / reject decisions all on the device; nothing crosses PCIe
 * between trials (extension: backend.py:101-103 is an empty class over a Map of
 * NUM_ACTIVE_KEYFRAMES = 7 keyframes, backend.py:11).  For windows of at most SLAM_BA_LM_MAX_FREE moving poses (a 96 x 96
 * system), 64 poses and SLAM_BA_LM_MAX_OBS observations; larger ones use slam_ba_reduce_f64 / slam_ba_backsub_f64 with
 * a host solve.
 *   d_poses2  [2][K,12]  in: the state in the first half;  d_points2 [2][L,3] likewise.  out: the optimised state is in
 *             half `d_stats[6]` of both (the halves swap roles on every accepted step).
 *   index tables as slam_ba_reduce_f64 (obs_pose / obs_point [O], pt_ptr [L+1] / pt_obs [O], ps_ptr [K+1] / ps_obs [O]);
 *             a (pose, point) pair may be observed once; the (pose, point) -> observation table is built on the device.  A
 *             pose or point index outside the window, a free list that is not ascending below K, or pose list heads that
 *             are not 0 = ps_ptr[0] <= ... <= ps_ptr[K] = O are counted (slam_index_errors) and end the launch (status 2);
 *             pt_ptr and the two observation lists are trusted (slam_ba_optimize_host_f64 builds all of them itself).
 *   d_free_poses int32 [n_free], ascending: the poses that move (the others hold the gauge).
 *   d_work    scratch of slam_ba_optimize_workspace(K, L, O) bytes, 16-byte aligned.
 *   d_stats   double [8]: initial cost, final cost, accepted steps, trials, final lambda, status (0 = ok; all NaN until the
 *             launch has completed; 1 = abandoned at a grid barrier: device busy; 2 = bad index / table), result half,
 *             workgroups used.
 * Schedule: lambda0 = 1e-5 max diag(H of the free poses and of the points); `iterations` iterations of up to 10 trials;
 * rho = (cost - cost_new) / (dx.(lambda dx - b) + 1e-3); accepted: lambda *= max(1/3, min(1 - (2 rho - 1)^3, 2/3));
 * rejected (or a factorisation that fails): lambda *= ni, ni *= 2.  Every sum is formed in a fixed order: two runs
 * give identical bits.  Asynchronous on the ctx stream.  The launch holds one compute unit per workgroup (at most 128, see
 * d_stats[7]) from start to end and needs all of them resident at once: launches of other contexts run beside it while
 * their workgroups fit as well (two of the largest do).  A launch larger than the device could ever hold is refused
 * (SLAM_ERR_BUSY); one that cannot get its workgroups resident NOW - other work holds compute units - gives up at a barrier
 * after 50 ms of wall clock and reports status 1, which slam_ba_optimize_host_f64 returns as SLAM_ERR_BUSY: the window is
 * unchanged and slam_ba_reduce_f64 / slam_ba_backsub_f64 (no residency requirement) do the same job. */
#define SLAM_BA_LM_MAX_FREE 16
#define SLAM_BA_LM_MAX_OBS (1 << 17)
SLAM_API int slam_ba_optimize_workspace(int64_t K, int64_t L, int64_t O, uint64_t* bytes);
/* The launch shape slam_ba_optimize_f64 takes for a window of K poses, O observations and n_free moving poses, WITHOUT a
 * device: *blocks workgroups, and every pose or pair task cut into *slices parts.  SLAM_ERR_INVALID for the sizes
 * slam_ba_optimize_f64 refuses. */
SLAM_API int slam_ba_optimize_shape(int64_t K, int64_t O, int64_t n_free, int32_t* blocks, int32_t* slices);
SLAM_API int slam_ba_optimize_f64(slam_ctx* ctx, int64_t K, int64_t L, int64_t O, const int32_t* d_obs_pose,
                                  const int32_t* d_obs_point, const double* d_meas, const int32_t* d_pt_ptr,
                                  const int32_t* d_pt_obs, const int32_t* d_ps_ptr, const int32_t* d_ps_obs,
                                  const int32_t* d_free_poses, int64_t n_free, double fx, double fy, double cx, double cy,
                                  double huber_delta, int iterations, double* d_poses2, double* d_points2, void* d_work,
                                  uint64_t work_bytes, double* d_stats);
/* slam_ba_optimize_f64 on HOST buffers: poses [K,12] and points [L,3] in, the optimised ones out; the index tables the kernel
 * wants are built inside (two stable counting sorts), a (pose, point) pair observed twice or an index out of range is
 * refused (SLAM_ERR_INVALID) before anything is launched; SLAM_ERR_BUSY = the launch gave up at a grid barrier (see above),
 * the outputs are not written.  h_pose_fixed [K]: non-zero = the pose holds the gauge.  One
 * upload, one launch, one download; staging, device arena and workspace belong to the context.  h_stats as d_stats above.
 * Serialises with the other host-buffer calls of the context. */
SLAM_API int slam_ba_optimize_host_f64(slam_ctx* ctx, int64_t K, int64_t L, int64_t O, const double* h_poses,
                                       const double* h_points, const int32_t* h_obs_pose, const int32_t* h_obs_point,
                                       const double* h_meas, const uint8_t* h_pose_fixed, double fx, double fy, double cx,
                                       double cy, double huber_delta, int iterations, double* h_poses_out,
                                       double* h_points_out, double* h_stats);

/* ---- SE(3) pose-graph optimisation (pose_graph.hip) -----------------------------------------------------------------
 * What pose_graph_sphere_example.py does with g2o: a graph of VertexSE3 / EdgeSE3 (:24-28, :45-52), vertex 0 fixed
 * (:29-30), Levenberg-Marquardt (:7) for 15 iterations (:57).  The block solver with a sparse direct factorisation
 * (BlockSolverSE3(LinearSolverEigenSE3()), :7) is replaced by conjugate gradients with a block-Jacobi preconditioner.
 *
 * Conventions.  Poses T = [R|t], [12] row-major 3x4, X_cam = R X_world + t; tangent vectors [w, v], rotation first; the
 * update is T <- Exp(d) T (as slam_pose_optimize_f64).
 *   measurement   edge (i, j) carries Z_ij [12], a measured value of T_j T_i^-1 (what recover_pose gives: X2 = R X1 + t)
 *   residual      r_ij = Log(T_j T_i^-1 Z_ij^-1) in R^6, the full SE(3) logarithm
 *   cost          F = sum rho(r^T Omega r), no factor 1/2 (g2o's chi2); Omega [36] symmetric, [w, v] order; rho = identity,
 *                 or Huber with huber_delta > 0 applied as slam_pose_optimize_f64 applies it (weight delta / sqrt(chi2))
 *   Jacobians     dr/dd_j = Jl^-1(r), dr/dd_i = -Jl^-1(r) Ad(T_j T_i^-1), Ad([R|t]) = [[R, 0], [t^ R, R]], Jl^-1 the exact
 *                 inverse left Jacobian of SE(3)
 *   system        H = sum w J^T Omega J, b = sum w J^T Omega r (no factor 2), solved as (H + lambda I) d = -b
 *   fixed         uint8 [V]; fixed poses come back bit for bit, their rows and columns leave the system; a graph without
 *                 a fixed vertex is SLAM_ERR_INVALID
 *   LM            g2o's schedule as slam_pose_optimize_f64 restates it: lambda_0 = 1e-5 * largest diagonal entry, the
 *                 gain-ratio update, ten trials per iteration before giving up
 * Relation to g2o (PARITY UNPINNED: g2o is absent): with X = T^-1 and Z_g = Z^-1, EdgeSE3's Z_g^-1 X_i^-1 X_j is the
 * inverse of T_j T_i^-1 Z^-1, so r is minus g2o's error taken as a logarithm and the information matrix carries over;
 * EdgeSE3 orders its error [translation, quaternion vector part], so a g2o file's 6x6 is permuted to rotation first and
 * scaled for q ~ w/2 (Omega_ww = Omega_qq / 4, Omega_wv = Omega_qv / 2) - slamhip.read_g2o does it.
 *
 * Vertex lists (device form): d_vtx_ptr [V+1], d_vtx_adj [2E]; the slots [ptr[v], ptr[v+1]) of vertex v hold 2 e + side
 * for every edge e that has v as its i (side 0) or j (side 1), in the order the sums are to be taken (the host form uses
 * ascending edge index).  Limits: V <= 2^24, E <= 2^25 (int32 indices).  Edge indices outside [0, V), self-edges and lists
 * that do not match the edges are found on the device before any kernel follows them: SLAM_ERR_INVALID, outputs untouched.
 * All arithmetic is f64 without contraction and without floating-point atomics: results are pure functions of the inputs.
 * Workspace: the context's grow-only block; the calls serialise on the context's call lock.  Angles of r beyond 3.1 rad
 * are outside the contract and reported (SLAM_PG_STATUS_ANGLE) instead of producing NaN.  An edge that is reported - its
 * angle beyond 3.1 rad, a pose or measurement that is not finite, or a robust cost that is not finite (an inf or NaN in
 * Omega) - leaves the sums: it adds 0 to the cost, and its W_e and its shares of H_vv and b are finite zeros. */
#define SLAM_PG_MAX_VERTICES (1 << 24)
#define SLAM_PG_MAX_EDGES (1 << 25)
#define SLAM_PG_STATUS_INDEX 1      /* bad edge index / vertex list (the call returns SLAM_ERR_INVALID) */
#define SLAM_PG_STATUS_ANGLE 2      /* a residual's rotation angle is beyond 3.1 rad: that edge was given weight 0 */
#define SLAM_PG_STATUS_PRECOND 4    /* a diagonal block H_vv + lambda I was not positive definite (identity used) */
#define SLAM_PG_STATUS_BREAKDOWN 8  /* CG met p.Ap <= 0 and stopped */
#define SLAM_PG_STATUS_NONFINITE 16 /* a non-finite cost, right-hand side or CG scalar */
/* bytes of context workspace a graph of V vertices and E edges takes; needs no device */
SLAM_API int slam_pg_workspace(int64_t V, int64_t E, uint64_t* bytes);
/* the launch plan, without a device: plan[8] = {blocks of the product's main path (= partial sums per dot product),
 * extra blocks for hub vertices, vertices per block (six lanes each), slots above which a vertex is a hub, blocks of the
 * edge kernel, CG iterations between two reads of the done flag, launches per CG iteration, 0} */
SLAM_API int slam_pg_plan(int64_t V, int64_t E, int32_t* plan);
/* Linearisation at d_poses: *d_cost = F, d_grad [V,6] = b, d_Hdiag [V,36] = the diagonal blocks H_vv, d_W [E,36] = the
 * off-diagonal blocks w J_i^T Omega J_j (row block i, column block j).  *h_status = SLAM_PG_STATUS_* bits (the call waits). */
SLAM_API int slam_pg_linearize_f64(slam_ctx* ctx, int64_t V, int64_t E, const double* d_poses, const int32_t* d_edges,
                                   const double* d_meas, const double* d_info, const int32_t* d_vtx_ptr,
                                   const int32_t* d_vtx_adj, double huber_delta, double* d_cost, double* d_grad,
                                   double* d_Hdiag, double* d_W, int32_t* h_status);
/* d_y [V,6] = (H + lambda I) d_x restricted to the free vertices (rows of fixed vertices 0, their columns ignored), H given
 * by d_Hdiag and d_W as slam_pg_linearize_f64 leaves them.  d_Hdiag and d_x 16-byte aligned. */
SLAM_API int slam_pg_hmul_f64(slam_ctx* ctx, int64_t V, int64_t E, const int32_t* d_edges, const int32_t* d_vtx_ptr,
                              const int32_t* d_vtx_adj, const uint8_t* d_fixed, const double* d_Hdiag, const double* d_W,
                              double lambda, const double* d_x, double* d_y);
/* Preconditioned CG on (H + lambda I) x = -d_b over the free vertices, stopping at |r| <= tol |b| or max_iter; alpha, beta
 * and the stop decision stay on the device.  h_stats[4] = {iterations, converged, |r| / |b| of the recurrence, status}.
 * converged = 1 exactly when the tolerance was met: a finite |r|^2 <= tol^2 |b|^2 (b = 0 meets it with x = 0 and no iteration).  A solve that stopped for
 * another reason - max_iter, SLAM_PG_STATUS_BREAKDOWN, a b or a CG scalar that is not finite - reports 0, and a |b| that is
 * not finite reports a |r| / |b| that is not finite. */
SLAM_API int slam_pg_pcg_f64(slam_ctx* ctx, int64_t V, int64_t E, const int32_t* d_edges, const int32_t* d_vtx_ptr,
                             const int32_t* d_vtx_adj, const uint8_t* d_fixed, const double* d_Hdiag, const double* d_W,
                             const double* d_b, double lambda, double tol, int max_iter, double* d_x, double* h_stats);
/* optimizer.optimize(15) of pose_graph_sphere_example.py:56-57 on device buffers.  n_fixed: how many entries of d_fixed are
 * non-zero (>= 1, checked against the mask on the device).  h_stats[8] = {initial chi2, final chi2, accepted LM
 * iterations, LM trials, CG iterations in total, final lambda, status bits, 0}.  V = 0 or E = 0 is not an error (E = 0:
 * the poses are copied).  One host read-back per LM trial and one per 32 CG iterations. */
SLAM_API int slam_pg_optimize_f64(slam_ctx* ctx, int64_t V, int64_t E, const double* d_poses, const int32_t* d_edges,
                                  const double* d_meas, const double* d_info, const uint8_t* d_fixed, int64_t n_fixed,
                                  const int32_t* d_vtx_ptr, const int32_t* d_vtx_adj, int iterations, double huber_delta,
                                  double pcg_tol, int pcg_max_iter, double* d_poses_out, double* h_stats);
/* the same on HOST buffers (the loop of pose_graph_sphere_example.py:24-57 after the file is read): the vertex lists are
 * built inside, one upload, one download.  On SLAM_ERR_INVALID h_poses_out is not written. */
SLAM_API int slam_pg_optimize_host_f64(slam_ctx* ctx, int64_t V, int64_t E, const double* h_poses, const int32_t* h_edges,
                                       const double* h_meas, const double* h_info, const uint8_t* h_fixed, int iterations,
                                       double huber_delta, double pcg_tol, int pcg_max_iter, double* h_poses_out,
                                       double* h_stats);

/* ---- Sim(3) pose-graph optimisation (sim3_graph.hip) ---------------------------------------------------------------
 * ORB-SLAM's OptimizeEssentialGraph for this project's conventions: the 7-DoF graph that absorbs the scale drift of a
 * monocular map, and the consumer of slam_sim3_* models.  Structure, guarantees, LM schedule, Huber, vertex lists, limits,
 * workspace and call lock are those of the slam_pg_* section above with 7x7 blocks; what differs is stated here.
 *
 * Conventions.  A vertex is a similarity S = (s, R, t), X_cam = s R X_world + t, stored [13]: the row-major 3x4 [R|t], then
 * s (the model layout of slam_sim3_*: their output feeds these calls unchanged).
 *   composition   (s_a, R_a, t_a) o (s_b, R_b, t_b) = (s_a s_b, R_a R_b, s_a R_a t_b + t_a);  inverse (1/s, R^T, -R^T t / s)
 *   tangent       d = [w, v, sigma], rotation first and scale last, 7 numbers
 *   chart         Phi(d) = Exp_SE3(w, v) o Scale(e^sigma) = (e^sigma, Exp(w), V(w) v)
 *   update        S <- Phi(d) o S:  s' = e^sigma s, R' = Exp(w) R, t' = e^sigma Exp(w) t + V(w) v
 *   measurement   edge (i, j) carries Z_ij [13], a measured value of S_j S_i^-1;  D = S_j S_i^-1 Z^-1
 *   residual      r = Phi^-1(D) = [Log_SE3(R_D, t_D), log s_D] in R^7
 *   cost          F = sum rho(r^T Omega r), no factor 1/2; Omega [49] symmetric in [w, v, sigma] order; rho as slam_pg_*
 *   Jacobians     dr/dd_j = J_j = [[Jl^-1, Jl^-1 (0; t_D)], [0, 1]], Jl^-1 the SE(3) inverse left Jacobian at r_1..6;
 *                 dr/dd_i = -J_j Ad(A), A = S_j S_i^-1 = (s, R, t), Ad(A) = [[R, 0, 0], [t^ R, s R, -t], [0, 0, 1]]
 *   system        H = sum w J^T Omega J, b = sum w J^T Omega r, solved as (H + lambda I) d = -b
 *   fix_scale     (ORB-SLAM's mbFixScale) column 7 of both Jacobians is zeroed: b_sigma = 0, H_sigma,sigma = lambda, every
 *                 d_sigma = 0 and every s comes back bit for bit
 *   validity      s of both ends, of Z and of D must be finite and positive; otherwise the edge leaves the sums with finite
 *                 zeros, as an angle beyond 3.1 rad does, and SLAM_S3G_STATUS_SCALE is raised
 * The chart is the exact inverse of the retraction and reuses the SE(3) logarithm; with fix_scale, every s = 1 and a
 * block-diagonal Omega the problem is the slam_pg_* one.  It differs from g2o's Sim3::log at second order in sigma * v:
 * PARITY UNPINNED against g2o's EdgeSim3 / ORB-SLAM (absent here). */
#define SLAM_S3G_MAX_VERTICES (1 << 24)
#define SLAM_S3G_MAX_EDGES (1 << 25)
#define SLAM_S3G_STATUS_INDEX 1      /* bad edge index / vertex list (the call returns SLAM_ERR_INVALID) */
#define SLAM_S3G_STATUS_ANGLE 2      /* a residual's rotation angle is beyond 3.1 rad: that edge was given weight 0 */
#define SLAM_S3G_STATUS_PRECOND 4    /* a diagonal block H_vv + lambda I was not positive definite (identity used) */
#define SLAM_S3G_STATUS_BREAKDOWN 8  /* CG met p.Ap <= 0 and stopped */
#define SLAM_S3G_STATUS_NONFINITE 16 /* a non-finite cost, right-hand side or CG scalar */
#define SLAM_S3G_STATUS_SCALE 32     /* a scale (vertex, measurement or their product) not finite and positive: weight 0 */
/* bytes of context workspace a graph of V vertices and E edges takes; needs no device */
SLAM_API int slam_s3g_workspace(int64_t V, int64_t E, uint64_t* bytes);
/* the launch plan, without a device: plan[8] = {blocks of the product's main path (= partial sums per dot product),
 * extra blocks for hub vertices, vertices per block (seven lanes each, nine vertices per wave), slots above which a vertex
 * is a hub, blocks of the edge kernel, CG iterations between two reads of the done flag, launches per CG iteration,
 * doubles per stored row of a slot block} */
SLAM_API int slam_s3g_plan(int64_t V, int64_t E, int32_t* plan);
/* Linearisation at d_sims [V,13] (scale free): *d_cost = F, d_grad [V,7] = b, d_Hdiag [V,49] = the diagonal blocks H_vv,
 * d_W [E,49] = the off-diagonal blocks w J_i^T Omega J_j.  *h_status = SLAM_S3G_STATUS_* bits (the call waits). */
SLAM_API int slam_s3g_linearize_f64(slam_ctx* ctx, int64_t V, int64_t E, const double* d_sims, const int32_t* d_edges,
                                    const double* d_meas, const double* d_info, const int32_t* d_vtx_ptr,
                                    const int32_t* d_vtx_adj, double huber_delta, double* d_cost, double* d_grad,
                                    double* d_Hdiag, double* d_W, int32_t* h_status);
/* d_y [V,7] = (H + lambda I) d_x restricted to the free vertices (rows of fixed vertices 0, their columns ignored), H given
 * by d_Hdiag and d_W as slam_s3g_linearize_f64 leaves them.  No alignment beyond that of a double is asked for. */
SLAM_API int slam_s3g_hmul_f64(slam_ctx* ctx, int64_t V, int64_t E, const int32_t* d_edges, const int32_t* d_vtx_ptr,
                               const int32_t* d_vtx_adj, const uint8_t* d_fixed, const double* d_Hdiag, const double* d_W,
                               double lambda, const double* d_x, double* d_y);
/* Preconditioned CG on (H + lambda I) x = -d_b over the free vertices, as slam_pg_pcg_f64 (7x7 LDL^T block-Jacobi).
 * h_stats[4] = {iterations, converged, |r| / |b| of the recurrence, status}. */
SLAM_API int slam_s3g_pcg_f64(slam_ctx* ctx, int64_t V, int64_t E, const int32_t* d_edges, const int32_t* d_vtx_ptr,
                              const int32_t* d_vtx_adj, const uint8_t* d_fixed, const double* d_Hdiag, const double* d_W,
                              const double* d_b, double lambda, double tol, int max_iter, double* d_x, double* h_stats);
/* The LM loop on device buffers, as slam_pg_optimize_f64; fix_scale != 0 freezes every scale.  h_stats[8] = {initial chi2,
 * final chi2, accepted LM iterations, LM trials, CG iterations in total, final lambda, status bits, 0}.  V = 0 or E = 0 is
 * not an error (E = 0: the vertices are copied). */
SLAM_API int slam_s3g_optimize_f64(slam_ctx* ctx, int64_t V, int64_t E, const double* d_sims, const int32_t* d_edges,
                                   const double* d_meas, const double* d_info, const uint8_t* d_fixed, int64_t n_fixed,
                                   const int32_t* d_vtx_ptr, const int32_t* d_vtx_adj, int iterations, double huber_delta,
                                   double pcg_tol, int pcg_max_iter, int fix_scale, double* d_sims_out, double* h_stats);
/* the same on HOST buffers: the vertex lists are built inside (slots in ascending edge order), one upload, one download.
 * On SLAM_ERR_INVALID h_sims_out is not written. */
SLAM_API int slam_s3g_optimize_host_f64(slam_ctx* ctx, int64_t V, int64_t E, const double* h_sims, const int32_t* h_edges,
                                        const double* h_meas, const double* h_info, const uint8_t* h_fixed, int iterations,
                                        double huber_delta, double pcg_tol, int pcg_max_iter, int fix_scale,
                                        double* h_sims_out, double* h_stats);

/* ---- sparse bundle adjustment (ba_sparse.hip) --------------------------------------------------------------------------
 * The bundle adjustment behind a closed loop: the points are eliminated into a reduced camera system that exists only
 * where two free poses see a common point, in the layout slam_pg_pcg_f64 / slam_pg_hmul_f64 take - d_Hdiag [K,36],
 * d_W [E,36] over the covisibility edges (k1 < k2, row block k1, column block k2), the gradient d_b [K,6], the mask d_fixed -
 * and the driver solves (S + lambda I) dp = -b with slam_pg_pcg_f64 as it is.  Conventions, residual, Jacobians and Huber
 * weight are those of slam_ba_reduce_f64; poses [K,12], points [L,3], cost without a factor 1/2, update T <- Exp(dp) T.
 *   Hpl_o   = w Jp^T Jq (6x3 row-major, [O,18])        Hll_l [L,6] packed upper triangle, bl_l [L,3]
 *   Hpp_k   [K,21] packed upper triangle, bp_k [K,6]   E_l = (Hll_l + lambda I)^-1 [L,9], 0 for a point nobody observes
 *   W_e     = - sum_{pairs (a, b) of edge e} Hpl_a E_l Hpl_b^T
 *   Hdiag_k = Hpp_k - sum_{o of k} Hpl_o E_l Hpl_o^T   (no lambda: the solver adds lambda I)
 *   b_k     = bp_k - sum_{o of k} Hpl_o E_l bl_l       dl_l = - E_l (bl_l + sum_{o of l} Hpl_o^T dp_pose(o))
 * Index tables (int32, device): d_pt_ptr [L+1] / d_pt_obs [O] and d_ps_ptr [K+1] / d_ps_obs [O] list the observations of
 * every point and pose in the order their sums are taken; d_pair_ptr [E+1] / d_pair_a [P] / d_pair_b [P] list, per edge
 * (k1, k2), the observations (k1, l) and (k2, l) of every common point l (slamhip.covisibility builds them, ascending in l).
 * Summation orders: a point's sums run down its list; a pose's sums give thread t of 256 the entries t, t + 256, .., then
 * an xor tree inside each wave and the four waves in order; an edge's sum gives lane i of ONE wave the pairs i, i + 64, ..
 * and the same xor tree - a function of the pair count alone, for one pair or thousands.  f64 without contraction and
 * without floating-point atomics: results are pure functions of the inputs.  Every buffer is the caller's
 * (slam_bas_workspace: their total); no call here takes the context's call lock or waits; all are asynchronous on the
 * context's stream.  No index outside its range is dereferenced.  Counted (slam_index_errors), once each, by the first
 * phase that reads it: an entry of obs_pose / obs_point (slam_bas_linearize_f64) or of pair_a / pair_b outside its range, a
 * slice of pt_ptr or ps_ptr (slam_bas_linearize_f64) or of pair_ptr that is negative, descending or ends past its table.
 * Not counted: an entry of pt_obs / ps_obs outside [0, O).  A bad entry makes what it feeds NaN (Hpl_o, Hll_l, cost_k,
 * Hdiag_k, dl_l, W_e); a bad slice of pt_ptr / ps_ptr is an empty list (its sums are 0), one of pair_ptr makes W_e NaN.
 * Limits: K <= 2^24, E <= 2^25 (the solver's), L, O <= 2^28, P <= 2^30. */
#define SLAM_BAS_MAX_POINTS (1 << 28)
#define SLAM_BAS_MAX_OBS (1 << 28)
#define SLAM_BAS_MAX_PAIRS (1 << 30)
/* bytes of device memory one problem takes in all (tables, state and candidate, blocks, steps); needs no device */
SLAM_API int slam_bas_workspace(int64_t K, int64_t L, int64_t O, int64_t E, int64_t P, uint64_t* bytes);
/* the launch plan, without a device: plan[8] = {workgroups of the observation kernel, of the point kernels, of the pose
 * kernels (one per pose), of the edge kernel (a wave per edge, four to a workgroup), of the candidate kernel (= partial sums
 * of the gain-ratio denominator), threads per workgroup, lanes that share an edge's pairs, 0} */
SLAM_API int slam_bas_plan(int64_t K, int64_t L, int64_t O, int64_t E, int64_t P, int32_t* plan);
/* Linearisation at (d_poses, d_points): d_Hpl, d_Hll, d_bl, d_Hpp, d_bp, the robust cost per pose d_cost [K], and
 * d_scal[0] = the cost, d_scal[1] = the largest diagonal entry of the Hpp of the free poses and of every Hll. */
SLAM_API int slam_bas_linearize_f64(slam_ctx* ctx, int64_t K, int64_t L, int64_t O, const double* d_poses, const double* d_points,
                                    const int32_t* d_obs_pose, const int32_t* d_obs_point, const double* d_meas,
                                    const int32_t* d_pt_ptr, const int32_t* d_pt_obs, const int32_t* d_ps_ptr,
                                    const int32_t* d_ps_obs, const uint8_t* d_fixed, double fx, double fy, double cx, double cy,
                                    double huber_delta, double* d_Hpl, double* d_Hll, double* d_bl, double* d_Hpp, double* d_bp,
                                    double* d_cost, double* d_scal);
/* the robust cost alone at a state: d_cost [K] per pose, *d_total their sum (the sums of slam_bas_linearize_f64) */
SLAM_API int slam_bas_cost_f64(slam_ctx* ctx, int64_t K, int64_t L, int64_t O, const double* d_poses, const double* d_points,
                               const int32_t* d_obs_pose, const int32_t* d_obs_point, const double* d_meas,
                               const int32_t* d_ps_ptr, const int32_t* d_ps_obs, double fx, double fy, double cx, double cy,
                               double huber_delta, double* d_cost, double* d_total);
/* the reduced system at damping lambda from the blocks of slam_bas_linearize_f64: d_E [L,9], d_Ebl [L,3] = E bl,
 * d_Hdiag [K,36], d_W [E,36], d_b [K,6] (blocks of fixed poses are written too; the solver ignores them) */
SLAM_API int slam_bas_reduce_f64(slam_ctx* ctx, int64_t K, int64_t L, int64_t O, int64_t E, int64_t P, const int32_t* d_obs_point,
                                 const int32_t* d_pt_ptr, const int32_t* d_ps_ptr, const int32_t* d_ps_obs,
                                 const int32_t* d_pair_ptr, const int32_t* d_pair_a, const int32_t* d_pair_b, const double* d_Hpl,
                                 const double* d_Hll, const double* d_bl, const double* d_Hpp, const double* d_bp, double lambda,
                                 double* d_E, double* d_Ebl, double* d_Hdiag, double* d_W, double* d_b);
/* d_dl [L,3] from the pose steps d_dp [K,6] (0 for fixed poses, as slam_pg_pcg_f64 leaves them) */
SLAM_API int slam_bas_backsub_f64(slam_ctx* ctx, int64_t K, int64_t L, int64_t O, const int32_t* d_pt_ptr, const int32_t* d_pt_obs,
                                  const int32_t* d_obs_pose, const double* d_Hpl, const double* d_E, const double* d_bl,
                                  const double* d_dp, double* d_dl);
/* the candidate state T' = Exp(dp) T (fixed poses copied bit for bit), X' = X + dl, and *d_denominator =
 * sum dp.(lambda dp - bp) over the free poses + sum dl.(lambda dl - bl), through d_part [plan[4]] partial sums */
SLAM_API int slam_bas_candidate_f64(slam_ctx* ctx, int64_t K, int64_t L, const uint8_t* d_fixed, const double* d_poses,
                                    const double* d_points, const double* d_dp, const double* d_dl, const double* d_bp,
                                    const double* d_bl, double lambda, double* d_poses_out, double* d_points_out, double* d_part,
                                    double* d_denominator);
/* The stereo / weighted forms of the two phases that read a measurement (the edge model above; ba_stereo.hip): the argument
 * lists of their parents with d_meas3 [O,3], d_info [O], bf, delta_mono, delta_stereo in place of d_meas, huber_delta.  Same
 * kernels per phase, list orders, sums and index-error accounting (an information that is none counts once, with the
 * observation's indices); slam_bas_reduce_f64, _backsub_f64, _candidate_f64 and slam_pg_pcg_f64 take the blocks as they
 * are.  With every mr NaN, every s = 1 and delta_mono = huber_delta all outputs equal the parents' in value. */
SLAM_API int slam_bas_linearize_stereo_f64(slam_ctx* ctx, int64_t K, int64_t L, int64_t O, const double* d_poses,
                                           const double* d_points, const int32_t* d_obs_pose, const int32_t* d_obs_point,
                                           const double* d_meas3, const double* d_info, const int32_t* d_pt_ptr,
                                           const int32_t* d_pt_obs, const int32_t* d_ps_ptr, const int32_t* d_ps_obs,
                                           const uint8_t* d_fixed, double fx, double fy, double cx, double cy, double bf,
                                           double delta_mono, double delta_stereo, double* d_Hpl, double* d_Hll, double* d_bl,
                                           double* d_Hpp, double* d_bp, double* d_cost, double* d_scal);
SLAM_API int slam_bas_cost_stereo_f64(slam_ctx* ctx, int64_t K, int64_t L, int64_t O, const double* d_poses, const double* d_points,
                                      const int32_t* d_obs_pose, const int32_t* d_obs_point, const double* d_meas3,
                                      const double* d_info, const int32_t* d_ps_ptr, const int32_t* d_ps_obs, double fx, double fy,
                                      double cx, double cy, double bf, double delta_mono, double delta_stereo, double* d_cost,
                                      double* d_total);
/* the classification at a state, one thread per observation: d_chi2 [O] the weighted chi2 (no kernel), d_inlier u8 [O] the
 * inlier rule above.  An observation with an index outside its range has chi2 NaN and is no inlier; it is not counted here. */
SLAM_API int slam_bas_classify_stereo_f64(slam_ctx* ctx, int64_t K, int64_t L, int64_t O, const double* d_poses,
                                          const double* d_points, const int32_t* d_obs_pose, const int32_t* d_obs_point,
                                          const double* d_meas3, const double* d_info, double fx, double fy, double cx, double cy,
                                          double bf, double chi2_mono, double chi2_stereo, double* d_chi2, uint8_t* d_inlier);

/* ---- bag-of-words place recognition (bow.hip) --------------------------------------------------------------
 * DBoW2's vocabulary tree, BoW vectors and inverted-file database for 256-bit descriptors, as ORB-SLAM's KeyFrameDatabase
 * uses them; no call site in the reference (it detects no loops).  PARITY UNPINNED: no DBoW2 exists here.  The tree is flat:
 * d_node_desc u8 [n_nodes,32], d_child int32 [n_nodes,2] = (first child, child count; 0 = leaf, children contiguous),
 * d_word_of_node int32 [n_nodes] (-1 for inner nodes), node 0 the root.  All buffers are the caller's; nothing is kept
 * between launches, and no call takes the context's call lock. */
/* h_limits [7] = {largest k, largest depth, descriptors per image, results per query, database entries per LDS pass of the
 * query, node rows the transform stages in LDS, descriptors up to which lanes = 0 means sixteen lanes}; needs no GPU */
SLAM_API int slam_bow_limits(int32_t* h_limits);
/* TemplatedVocabulary::transform(feature, word id, node id, levelsup) for n descriptors u8 [n,32]: at every inner node to
 * the child at the smallest Hamming distance (lowest child on ties), d_words [n] the leaf's word, d_nodes [n] the node of
 * the path at depth min(leaf depth, max(0, depth - levels_up)).  lanes: 1 = one lane per descriptor (the tree's first 1152
 * rows staged in LDS), 16 = sixteen lanes per descriptor (one child per lane), 0 = chosen by n; the same results either way */
SLAM_API int slam_bow_transform(slam_ctx* ctx, const void* d_desc, int64_t n, const void* d_node_desc, const int32_t* d_child,
                                const int32_t* d_word_of_node, int64_t n_nodes, int depth, int levels_up, int lanes,
                                int32_t* d_words, int32_t* d_nodes);
/* TemplatedVocabulary::transform(features, BowVector) under TF_IDF + L1_NORM for B images: image b owns the word ids
 * d_words_in[d_offsets[b] .. d_offsets[b+1]) (at most 8192).  Output rows compressed: d_out_offsets int64 [B+1], and per kept
 * word (ascending id) its id, value f64 and q = floor(value * 2^31); the three output arrays hold n slots (the worst case).
 * d_ws: slam_bow_vectors_workspace(B, n) bytes. */
SLAM_API int slam_bow_vectors(slam_ctx* ctx, const int32_t* d_words_in, const int64_t* d_offsets, int64_t B, int64_t n,
                              const double* d_idf, int64_t n_words, void* d_ws, uint64_t ws_bytes, int64_t* d_out_offsets,
                              int32_t* d_out_words, double* d_out_values, uint32_t* d_out_q);
SLAM_API int slam_bow_vectors_workspace(int64_t B, int64_t n, uint64_t* h_bytes);
/* counting sort: d_perm lists the items i with 0 <= d_keys[i] < n_keys grouped by key, d_key_off int32 [n_keys+1] where each
 * group starts (the order inside a group is unspecified); d_cursor int32 [n_keys] is scratch */
SLAM_API int slam_bow_group_keys(slam_ctx* ctx, const int32_t* d_keys, int64_t n, int64_t n_keys, int32_t* d_key_off,
                                 int32_t* d_cursor, int32_t* d_perm);
/* the inverted file of TemplatedDatabase (m_ifile) from the forward store: T (word, entry id, q) triples -> d_word_off int32
 * [n_words+1] and d_postings [T] of (entry id, q) u32 pairs grouped by word; d_cursor [n_words] and d_perm [T] are scratch */
SLAM_API int slam_bow_index_build(slam_ctx* ctx, const int32_t* d_words, const int32_t* d_entry, const uint32_t* d_q, int64_t T,
                                  int64_t n_words, int32_t* d_word_off, int32_t* d_cursor, int32_t* d_perm, void* d_postings);
/* TemplatedDatabase::queryL1 in fixed point for Q vectors (rows as slam_bow_vectors writes them): s_int = sum over the shared
 * words of min(q, p), common = their number.  Top form (d_dense_s null): per query the entries with id < max_id that share a
 * word, by (s_int descending, id ascending), the first max_results (<= 64) into d_ids / d_s_int / d_common [Q,max_results],
 * fillers (-1, 0, 0).  Dense form (both d_dense_* given): s_int and common of every entry, [Q,E]; max_id, max_results and the
 * three top tables are ignored. */
SLAM_API int slam_bow_query(slam_ctx* ctx, const int64_t* d_q_offsets, const int32_t* d_q_words, const uint32_t* d_q_q, int64_t Q,
                            const int32_t* d_word_off, const void* d_postings, int64_t n_words, int64_t E, int64_t max_id,
                            int max_results, int32_t* d_ids, uint32_t* d_s_int, int32_t* d_common, uint32_t* d_dense_s,
                            int32_t* d_dense_common);
/* Training, one depth of the tree per round (TemplatedVocabulary::HKmeansStep for all nodes of a depth at once; maximin
 * seeding instead of k-means++).  d_row_node int32 [n]: the node (index within the depth, < F) of each row, -1 = at a leaf;
 * node f owns the centre rows d_cent u8 [F,k,32], d_cent_count [F] of them in use.
 * seed: centre 0 = the node's first row, each further one the row farthest from the centres so far (first row on ties),
 * until k centres or distance 0.  d_ws: slam_bow_train_seed_workspace(n, F) bytes. */
SLAM_API int slam_bow_train_seed(slam_ctx* ctx, const void* d_desc, int64_t n, const int32_t* d_row_node, int64_t F, int k,
                                 void* d_cent, int32_t* d_cent_count, void* d_ws, uint64_t ws_bytes);
SLAM_API int slam_bow_train_seed_workspace(int64_t n, int64_t F, uint64_t* h_bytes);
/* step: d_assign [n] = nearest centre of each live row (lowest index on ties), *h_changed = rows whose assignment changed
 * (waits for the stream); with `update` and *h_changed > 0 every centre that has rows becomes their bitwise majority (a bit is
 * set iff 2 * count >= rows, DBoW2's meanValue).  d_perm: the n_live live rows grouped by node (slam_bow_group_keys on
 * d_row_node); d_bits u32 [F,k,256], d_rows_of u32 [F,k] and d_changed u32 [1] are scratch. */
SLAM_API int slam_bow_train_step(slam_ctx* ctx, const void* d_desc, int64_t n, const int32_t* d_row_node, int64_t F, int k,
                                 void* d_cent, const int32_t* d_cent_count, int32_t* d_assign, const int32_t* d_perm,
                                 int64_t n_live, uint32_t* d_bits, uint32_t* d_rows_of, uint32_t* d_changed, int update,
                                 int64_t* h_changed);
/* descend: with d_own (u32 [F,k]) the rows each centre owns; with d_next_of (int32 [F,k]) d_row_node[i] becomes
 * d_next_of[node, assignment], the row's node of the next depth (-1 = at a leaf).  Exactly one of the two. */
SLAM_API int slam_bow_train_descend(slam_ctx* ctx, int32_t* d_row_node, const int32_t* d_assign, int64_t n, int64_t F, int k,
                                    uint32_t* d_own, const int32_t* d_next_of);

/* ---- node-constrained matching over the BoW direct index (bow_match.hip) -----------------------------------
 * ORBmatcher::SearchByBoW: the correspondences of candidate image pairs, comparing only the features that slam_bow_transform
 * (bow_transform(..., levels_up)) put into the same vocabulary node; no call site in the reference.  PARITY UNPINNED: the
 * one-to-one step and the rotation check are stated on integers (4k).  A pair is (side 1 = the keyframe, side 2 = the frame);
 * row j of side 2 is a candidate for row i of side 1 iff their node ids are equal and >= 0 (a negative id takes a row out of
 * the search on either side).  At most SLAM_BOW_MATCH_ROWS_MAX rows per image and SLAM_BOW_MATCH_PAIRS_MAX pairs per call. */
#define SLAM_BOW_MATCH_ROWS_MAX 8192
#define SLAM_BOW_MATCH_PAIRS_MAX 4096
/* h_limits [6] = {rows per image, pairs per call, threads of a group workgroup, side-1 rows of a scan workgroup, orientation
 * bins, the distance a missing second neighbour counts as in the ratio test}; needs no GPU */
SLAM_API int slam_bow_match_limits(int32_t* h_limits);
/* The launch plan for B images (group) or B pairs (search) of n rows per image; needs no GPU.  h_plan [8] = {length of the
 * LDS sort (n padded to a power of two), LDS bytes of a group workgroup, group workgroups, scan workgroups, finish workgroups,
 * workspace bytes of the search when the tables stay in the workspace, LDS bytes of a finish workgroup, workspace bytes of
 * the group step} */
SLAM_API int slam_bow_match_plan_describe(int64_t B, int64_t n, int64_t* h_plan);
/* The group step - DBoW2's FeatureVector of B images at once, built once per image and reused by every search: image b owns the
 * rows [h_offsets[b], h_offsets[b+1]) of d_desc u8 [n,32] and of d_nodes int32 [n] (slam_bow_transform's d_nodes; h_offsets
 * is a HOST array and travels through the context's workspace).  Inside each image the rows are sorted by (node id as
 * unsigned 32-bit, row), so masked rows go last: d_order [n] the row (local to its image) at each position, d_nodes_sorted
 * [n] its node id, d_desc_sorted [n,32] its descriptor, d_inverse [n] the position of each row.  Asynchronous on the ctx
 * stream. */
SLAM_API int slam_bow_match_group(slam_ctx* ctx, const void* d_desc, const int32_t* d_nodes, const int64_t* h_offsets, int64_t B,
                                  void* d_desc_sorted, int32_t* d_nodes_sorted, int32_t* d_order, int32_t* d_inverse);
/* one set of grouped images, as slam_bow_match_group leaves it; d_bins: the orientation bin (0 .. 31, taken modulo 32) of each
 * row in ROW order, or null; h_offsets is a HOST array */
typedef struct slam_bow_groups {
    const void* d_desc;
    const int32_t* d_nodes;
    const int32_t* d_order;
    const int32_t* d_inverse;
    const uint8_t* d_bins;
    const int64_t* h_offsets;
    int64_t B;
} slam_bow_groups;
/* The node top-2 of P pairs: h_pairs is a HOST array int32 [P,2] of (image of g1, image of g2); the pair table travels through
 * the context's workspace.  Per side-1 row its two nearest candidates by (distance, side-2 row), rows local to the pair's
 * images, missing neighbours (-1, INT32_MAX): d_idx / d_dist int32 [sum of the pairs' side-1 rows, 2], pair after pair in
 * row order.  With all node ids equal this is slam_bf_knn2_u256.  scan_order: 0 = a lane per grouped position (shipped),
 * 1 = a lane per row; the same results.  Asynchronous on the ctx stream (the table is copied from pageable host memory as
 * slam_upload copies: the runtime may hold the caller until that copy has run; the launches behind it are not waited for). */
SLAM_API int slam_bow_match_top2(slam_ctx* ctx, const slam_bow_groups* g1, const slam_bow_groups* g2, const int32_t* h_pairs, int64_t P,
                                 int scan_order, int32_t* d_idx, int32_t* d_dist);
/* ORBmatcher::SearchByBoW for P pairs: the node top-2, then row i is proposed iff d0 <= th_low and (double)d0 < ratio * (double)d1
 * (a missing second neighbour counts as 256); among the proposed rows that name one side-2 row the smallest (d0, i) keeps it;
 * and, when both sets carry bins, the rotation check: the histogram of (bin1[i] - bin2[j]) & 31, of which the first bin by
 * (count descending, bin ascending) stays, and the second and third while their count c > 0 and 10 c >= the first's.
 * d_matches12 int32 [sum of side-1 rows]: the side-2 row of each side-1 row or -1 (vpMatches12), d_count int32 [P] the matches
 * of each pair; d_idx / d_dist: the top-2 tables as slam_bow_match_top2 writes them, or both null.  No host read-back between
 * the steps; asynchronous on the ctx stream. */
SLAM_API int slam_bow_match_search(slam_ctx* ctx, const slam_bow_groups* g1, const slam_bow_groups* g2, const int32_t* h_pairs, int64_t P,
                                   int th_low, double ratio, int scan_order, int32_t* d_matches12, int32_t* d_count, int32_t* d_idx,
                                   int32_t* d_dist);

/* ---- map points matched into frames by projection (proj_match.hip) ------------------------------------------
 * ORBmatcher::SearchByProjection (the forms TrackWithMotionModel, TrackLocalMap / SearchLocalPoints, Relocalization and
 * ComputeSim3 call) for up to SLAM_PROJ_MATCH_PAIRS_MAX (point set, frame, pose) pairs a call; the reference tracks by a
 * whole-image brute-force match instead (frontend.py:156-187).  PARITY UNPINNED: the gates are stated in f64 in a fixed
 * operation order, the predicted level without log, the one-to-one step and the rotation check as in 4k. */
#define SLAM_PROJ_MATCH_ROWS_MAX 8192
#define SLAM_PROJ_MATCH_PAIRS_MAX 4096
#define SLAM_PROJ_MATCH_LEVELS_MAX 16
/* h_limits [6] = {rows per frame and points per set, pairs per call, points of a scan workgroup, pyramid levels, orientation
 * bins, bytes of one pair record in the workspace}; needs no GPU */
SLAM_API int slam_proj_match_limits(int32_t* h_limits);
/* The launch plan for B frames (grid step) and P pairs (search) of n rows / points each; needs no GPU.  h_plan [8] = {cell
 * workgroups, sort workgroups, gather workgroups, scan workgroups, finish workgroups, workspace bytes of the search when the
 * top-2 tables stay in the workspace, LDS bytes of a finish workgroup, workspace bytes of the grid step} */
SLAM_API int slam_proj_match_plan_describe(int64_t B, int64_t P, int64_t n, int64_t* h_plan);
/* The grid step - Frame::AssignFeaturesToGrid for B frames at once, built once per frame and reused by every search: frame b
 * owns the rows [h_offsets[b], h_offsets[b+1]) (h_offsets a HOST array) of d_desc u8 [n,32], d_xy f32 [n,2] (level-0 pixels),
 * d_level int32 [n] and d_taken u8 [n] (non-zero: out of every search; may be null).  The rows fall into square cells of
 * `cell` pixels over [0, W) x [0, H), indices clamped into the grid; d_cells [n] receives each row's cell id, and inside each
 * frame the rows are sorted by (cell, row): d_order the row at each position, d_cells_sorted, d_desc_sorted, d_xy_sorted and
 * d_meta_sorted (the level, -1 for a taken row) the same order, d_inverse the position of each row.  Asynchronous on the ctx
 * stream. */
SLAM_API int slam_proj_match_grid(slam_ctx* ctx, const void* d_desc, const float* d_xy, const int32_t* d_level, const uint8_t* d_taken,
                                  const int64_t* h_offsets, int64_t B, int W, int H, int cell, int32_t* d_cells, void* d_desc_sorted,
                                  int32_t* d_cells_sorted, int32_t* d_order, int32_t* d_inverse, float* d_xy_sorted,
                                  int32_t* d_meta_sorted);
/* one set of frames as slam_proj_match_grid leaves it; d_level and d_bins (orientation bins, or null) in ROW order */
typedef struct slam_proj_frames {
    const void* d_desc;
    const int32_t* d_cells;
    const int32_t* d_order;
    const float* d_xy;
    const int32_t* d_meta;
    const int32_t* d_level;
    const uint8_t* d_bins;
    const int64_t* h_offsets;
    int64_t B;
    int32_t W, H, cell, pad;
} slam_proj_frames;
/* map points (MapPoint): set a owns the points [h_offsets[a], h_offsets[a+1]); d_xyz f64 [n,3] world positions, d_desc u8
 * [n,32]; optional (null: the gate or rule is off): d_range f64 [n,2] = (dmin^2, dmax^2) of the scale-invariance distances
 * (MapPoint::GetMinDistanceInvariance / GetMaxDistanceInvariance, squared), d_normal f64 [n,3] (GetNormal), d_level int32 [n]
 * the level the point was last seen at (clamped into [0, n_levels)), d_bins u8 [n] */
typedef struct slam_proj_points {
    const double* d_xyz;
    const void* d_desc;
    const double* d_range;
    const double* d_normal;
    const int32_t* d_level;
    const uint8_t* d_bins;
    const int64_t* h_offsets;
    int64_t B;
} slam_proj_points;
/* camera, bounds, scale tables (HOST arrays of n_levels doubles: s^l and their squares) and the rules of one call; level_rule
 * non-zero: frame row j is a candidate only if lp + lo <= level_j <= lp + hi */
typedef struct slam_proj_params {
    double fx, fy, cx, cy;
    double min_x, max_x, min_y, max_y;
    double cos2_limit, ratio;
    const double* h_scale;
    const double* h_scale2;
    int32_t n_levels, th_high, level_rule, lo, hi, pad;
} slam_proj_params;
/* The gates alone (Frame::isInFrustum / the head of every SearchByProjection): for pair p the points of set h_sets[p] under the
 * pose h_poses[p] (f64 [P,3,4] row-major, world -> camera; a rigid pose or [sR | t]), the camera centre h_centres[p] and the
 * radius factor h_th[p] -> d_status (0 searched, 1 not in front, 2 out of bounds, 3 out of range, 4 off the normal), d_u, d_v
 * f64 (NaN where never computed) and d_lp (the predicted level, -1), pair after pair. */
SLAM_API int slam_proj_match_project(slam_ctx* ctx, const slam_proj_points* points, const int32_t* h_sets, const double* h_poses,
                                     const double* h_centres, const double* h_th, int64_t P, const slam_proj_params* params,
                                     int32_t* d_status, double* d_u, double* d_v, int32_t* d_lp);
/* ORBmatcher::SearchByProjection for P pairs h_pairs int32 [P,2] = (point set, frame): the gates; per surviving point its two
 * nearest frame rows by (distance, row) among the rows that are not taken, lie strictly inside the window of radius
 * h_th[p] * scale[lp] about (u, v) and pass the level rule; the selection d0 <= th_high and not (a second neighbour on the
 * first one's level with (double)d0 > ratio * (double)d1); the one-to-one step and the rotation check of
 * slam_bow_match_search.  d_matches12 int32 [sum of the pairs' points], d_count int32 [P]; the tables d_status / d_u / d_v /
 * d_lp (all or none) and d_idx / d_dist int32 [., 2] (both or neither) are optional.  The pair table and the parameters
 * travel through the context's workspace; one memset and two launches; no host read-back; asynchronous on the ctx stream. */
SLAM_API int slam_proj_match_search(slam_ctx* ctx, const slam_proj_points* points, const slam_proj_frames* frames, const int32_t* h_pairs,
                                    const double* h_poses, const double* h_centres, const double* h_th, int64_t P,
                                    const slam_proj_params* params, int32_t* d_matches12, int32_t* d_count, int32_t* d_status, double* d_u,
                                    double* d_v, int32_t* d_lp, int32_t* d_idx, int32_t* d_dist);

/* ---- epipolar node search and new map points (tri_match.hip) -----------------------------------------------
 * ORBmatcher::SearchForTriangulation and the per-match half of LocalMapping::CreateNewMapPoints for up to
 * SLAM_TRI_MATCH_PAIRS_MAX keyframe pairs a call; the reference creates its points from a whole-image match and a bare
 * triangulation (frontend.py).  PARITY UNPINNED: the gates are stated in f64 in a fixed operation order, the epipolar distance
 * without its division, the DLT by Jacobi sweeps instead of an SVD, the one-to-one step and the rotation check as in 4k. */
#define SLAM_TRI_MATCH_ROWS_MAX 8192
#define SLAM_TRI_MATCH_PAIRS_MAX 4096
#define SLAM_TRI_MATCH_LEVELS_MAX 16
/* h_limits [8] = {rows per image, pairs per call, rows of a scan workgroup, pyramid levels, orientation bins, bytes of one pair
 * record of the search, of the triangulation, bytes of the parameter block}; needs no GPU */
SLAM_API int slam_tri_match_limits(int32_t* h_limits);
/* The launch plan for P pairs of n rows per image; needs no GPU.  h_plan [6] = {scan workgroups, finish workgroups,
 * triangulation workgroups (256 rows each), workspace bytes of the search when the top-2 tables stay in the workspace, workspace bytes of the
 * triangulation, LDS bytes of a finish workgroup} */
SLAM_API int slam_tri_match_plan_describe(int64_t P, int64_t n, int64_t* h_plan);
/* what a keyframe's rows carry besides their descriptors, in ROW order over the whole set: d_xy f32 [n,2] level-0 pixels,
 * d_level int32 [n] pyramid levels (clamped into [0, n_levels)), d_taken u8 [n] or null: non-zero = the row has a map point
 * already and is out of the search (it is not the masking by a negative node id: the grouped set stays as it is) */
typedef struct slam_tri_views {
    const float* d_xy;
    const int32_t* d_level;
    const uint8_t* d_taken;
} slam_tri_views;
/* camera, gates and level tables (HOST arrays of n_levels doubles: scale[l] = s^l and sigma2[l] = scale[l]^2) of one call.
 * The search reads th_low, chi2, epipole_r2 and the tables; the triangulation the camera, cos_max, chi2_px, ratio_factor and
 * the tables. */
typedef struct slam_tri_params {
    double fx, fy, cx, cy;
    double chi2, epipole_r2;
    double cos_max, chi2_px, ratio_factor;
    const double* h_scale;
    const double* h_sigma2;
    int32_t n_levels, th_low;
} slam_tri_params;
/* ORBmatcher::SearchForTriangulation for P pairs h_pairs int32 [P,2] = (image of g1, image of g2), the sets as
 * slam_bow_match_search takes them.  h_F f64 [P,9]: F12 row-major, x1^T F12 x2 = 0; h_epipole f64 [P,2]: the epipole of camera 1
 * in image 2 (a NaN component: no epipole gate); both HOST arrays that travel with the pair table through the context's
 * workspace.  Row j of side 2 is a candidate for row i of side 1 iff node1[i] == node2[j] >= 0, neither row is taken, the
 * Hamming distance d <= th_low, NOT (ex - x2)^2 + (ey - y2)^2 < epipole_r2 * scale[l] with l = level2[j] clamped (ORB-SLAM's
 * 100 * scaleFactor: the scale, not its square), and with (a, b, c) = F12^T (x1, y1, 1), num = (a x2 + b y2) + c and
 * den = a a + b b: den > 0 and num num < (chi2 sigma2[l]) den (CheckDistEpipolarLine; strict, so F = 0 or a NaN passes
 * nothing).  Per side-1 row the two nearest candidates by (distance, side-2 row) -> d_idx / d_dist as slam_bow_match_top2
 * lays them out (both or neither); a row with a first neighbour is proposed (no ratio test: ORB-SLAM has none here); then the
 * one-to-one step and the rotation check of slam_bow_match_search -> d_matches12 int32 [sum of side-1 rows], d_count int32
 * [P].  One copy, one memset, two launches; no host read-back; asynchronous on the ctx stream. */
SLAM_API int slam_tri_match_search(slam_ctx* ctx, const slam_bow_groups* g1, const slam_bow_groups* g2, const slam_tri_views* views1,
                                   const slam_tri_views* views2, const int32_t* h_pairs, int64_t P, const double* h_F,
                                   const double* h_epipole, const slam_tri_params* params, int scan_order, int32_t* d_matches12,
                                   int32_t* d_count, int32_t* d_idx, int32_t* d_dist);
/* LocalMapping::CreateNewMapPoints behind its matching, for the same pairs over the same image offsets (HOST arrays): every
 * side-1 row i with d_matches12[i] = j in [0, n2) is triangulated from the poses h_T1, h_T2 (f64 [P,3,4] world -> camera) with
 * the camera centres h_O1, h_O2 (f64 [P,3]).  d_status int32: 0 created, 1 no match, 2 parallax (rays R^T xn: dot > 0 and
 * dot^2 < cos_max^2 n1 n2 required), 3 at infinity (the DLT's w <= 0 or X not finite), 4 / 5 not in front of camera 1 / 2,
 * 6 / 7 squared reprojection error > chi2_px sigma2[level] in image 1 / 2, 8 scale inconsistent (dist2 / dist1 against
 * scale[l1] / scale[l2] within ratio_factor); the first failure wins.  d_X f64 [.,3], d_normal f64 [.,3] (MapPoint::
 * UpdateNormalAndDepth with keyframe 1 as the reference) and d_range f64 [.,2] = (dmin^2, dmax^2) hold NaN wherever
 * status != 0: a NaN position fails the first gate of slam_proj_match_search, so the arrays are a slam_proj_points as they
 * stand, uncompacted.  d_created int32 [P]: the points of each pair.  One copy, one memset, one launch; asynchronous. */
SLAM_API int slam_tri_match_triangulate(slam_ctx* ctx, const int64_t* h_offsets1, int64_t B1, const int64_t* h_offsets2, int64_t B2,
                                        const slam_tri_views* views1, const slam_tri_views* views2, const int32_t* h_pairs, int64_t P,
                                        const int32_t* d_matches12, const double* h_T1, const double* h_T2, const double* h_O1,
                                        const double* h_O2, const slam_tri_params* params, double* d_X, double* d_normal,
                                        double* d_range, int32_t* d_status, int32_t* d_created);

/* ---- map-point fusion and observation refresh (fuse.hip) ----------------------------------------------------
 * ORBmatcher::Fuse (LocalMapping::SearchInNeighbors; LoopClosing::SearchAndFuse with [sR | t] poses) for up to
 * SLAM_PROJ_MATCH_PAIRS_MAX (point set, frame, pose) pairs a call, and MapPoint::ComputeDistinctiveDescriptors with
 * MapPoint::UpdateNormalAndDepth for the points it touched; the reference has neither.  PARITY UNPINNED: integers and f64 in a
 * fixed operation order; deterministic one-to-one and merge rules instead of iteration order, a unit normal instead of the
 * mean, the chi2 product instead of the division, at most SLAM_FUSE_OBS_MAX observations a point.
 * The observations of the M map points are one table in compressed rows: offsets int64 [M+1] (a HOST array and its copy on the
 * device) and d_obs int32 [nnz,2] = (frame, row inside that frame), the frames of one list strictly ascending. */
#define SLAM_FUSE_OBS_MAX 256
/* h_limits [8] = {rows per frame and points per set, pairs per call, points of a scan workgroup, pyramid levels, observations
 * per point, bytes of one pair record, bytes of one refresh job, threads of a refresh workgroup}; needs no GPU */
SLAM_API int slam_fuse_limits(int32_t* h_limits);
/* what the search takes beside a slam_proj_params (whose ratio, th_high and level_rule it does not read: there is no ratio
 * test, and the level rule is always on): the margins of the range gate, SQUARED (ORB-SLAM: 0.8^2, 1.2^2; both positive),
 * the chi2 of the reprojection gate (5.99) and the largest accepted descriptor distance (ORBmatcher::TH_LOW = 50) */
typedef struct slam_fuse_params {
    double m_lo2, m_hi2, chi2;
    int32_t th_low, pad;
} slam_fuse_params;
/* ORBmatcher::Fuse for P pairs h_pairs int32 [P,2] = (point set, frame).  d_id int32 [points]: the map point of each point
 * (-1: none); frames: a frame set as slam_proj_match_grid leaves it, built WITHOUT taken marks; d_point int32 [rows], ROW
 * order: the map point each frame row holds, or -1.  Per point, the first that applies: status 5 - its list (d_id >= 0) holds
 * an observation in the pair's frame; 1 - 4 - the gates of slam_proj_match_project, the range gate as d2 < m_lo2 dmin2 ||
 * d2 > m_hi2 dmax2, the level predicted from dmax2 itself; 6 - no candidate, a candidate being a frame row j strictly inside
 * the window of radius h_th[p] * scale[lp] with lp + lo <= level_j <= lp + hi and NOT e2 > chi2 * h_scale2[level_j] for
 * e2 = (u - x_j)^2 + (v - y_j)^2 in f64; 7 - the nearest candidate by (distance, row) is farther than th_low; 8 - another
 * point of the pair proposed the same row with a smaller (distance, point); 0 - linked.  d_row (-1 unless status 0, 7, 8),
 * d_dist (INT32_MAX where there is no row), d_status, d_other (status 0: d_point of the row - -1 = the point gains an
 * observation there, q >= 0 = the same landmark as q; status 8: d_id of the winner; else -1) int32 [sum of the pairs' points],
 * pair after pair; d_count int32 [P,3] = status-0 rows with other < 0, status-0 rows with other >= 0, status-8 rows; d_u,
 * d_v f64 and d_lp int32 optional (all or none).  One copy, one memset, two launches; asynchronous on the ctx stream. */
SLAM_API int slam_fuse_search(slam_ctx* ctx, const slam_proj_points* points, const int32_t* d_id, const slam_proj_frames* frames,
                              const int32_t* d_point, const int64_t* h_obs_offsets, const int64_t* d_obs_offsets, const int32_t* d_obs,
                              int64_t M, const int32_t* h_pairs, const double* h_poses, const double* h_centres, const double* h_th, int64_t P,
                              const slam_proj_params* params, const slam_fuse_params* fuse, int32_t* d_row, int32_t* d_dist,
                              int32_t* d_status, int32_t* d_other, int32_t* d_count, double* d_u, double* d_v, int32_t* d_lp);
/* The refresh of K map points, h_select int32 [K] of the M (null: all M, K ignored), results in that order.  d_xyz f64 [M,3];
 * the frames' descriptors d_desc u8 [n,32] and levels d_level int32 [n] in ROW order over the B frames of h_frame_offsets
 * (d_inverse non-null: d_desc is in grid order and d_inverse the grid position of each row, as slam_proj_match_grid leaves
 * them); d_centres f64 [B,3] the camera centres; d_ref int32 [M] the index inside its list of each point's reference
 * observation (clamped into the list; null: 0); h_scale f64 [n_levels].  With N the length of a list: D[i][k] the Hamming
 * distance of observations i and k, med_i the element of rank (N - 1) / 2 of row i ascending, d_best the smallest (med_i, i)
 * and d_desc_out u8 [K,32] its descriptor; d_normal f64 [K,3] = unit(sum over the list, in list order, of (X - O) / |X - O|);
 * d_range f64 [K,2] = (dmin^2, dmax^2), dmax = |X - O_ref| * scale[level_ref], dmin = dmax / scale[n_levels - 1].  N = 0: -1,
 * zero bytes, NaN; a normal that is not finite: NaN normal and range, the descriptor still chosen.  Up to three launches by
 * list length (16, 64, 256 lanes a point); asynchronous on the ctx stream. */
SLAM_API int slam_fuse_refresh(slam_ctx* ctx, const double* d_xyz, const int64_t* h_obs_offsets, const int32_t* d_obs, int64_t M,
                               const int32_t* h_select, int64_t K, const void* d_desc, const int32_t* d_inverse, const int32_t* d_level,
                               const int64_t* h_frame_offsets, int64_t B, const double* d_centres, const int32_t* d_ref, const double* h_scale,
                               int n_levels, int32_t* d_best, void* d_desc_out, double* d_normal, double* d_range);

/* ---- the covisibility graph (covis.hip) ----------------------------------------------------------------------
 * slamhip.covisibility on the device, bit for bit (KeyFrame::UpdateConnections for the whole map at once; the reference has
 * no covisibility graph).  From d_obs_pose / d_obs_point int32 [O] and a byte mask d_fixed [K] (null: every pose counts):
 *   d_edges int32 [E,2], k1 < k2, every pair of free poses with a common point, ascending by (k1, k2); d_weights int32 [E];
 *   d_pair_ptr int32 [E+1]; d_pair_a / d_pair_b int32 [P]: the observation indices of (k1, l) and (k2, l), ascending in l.
 * Three phases, because the host sizes the tables of each from the scalars of the one before:
 *   slam_covis_count   sorts the observations by (point, fixed, pose) and scans the pairs of every point; waits, and returns
 *                      h_scalars [4] = {observations of free poses, (pose, point) pairs observed more than once (fixed poses
 *                      included), P, entries of obs_pose / obs_point out of range (also in slam_index_errors; such an entry
 *                      is never dereferenced and takes no part)}.  With duplicates the later phases must not run.
 *   slam_covis_pairs   writes the P pairs in point order, sorts them by k1 K + k2 (stable, 8-bit digits over the bits of
 *                      K^2 - 1; 64-bit keys above K = 65 536) into d_pair_a / d_pair_b, counts the edges; waits, returns *h_edges.
 *   slam_covis_edges   writes d_edges, d_weights and d_pair_ptr (E as returned); asynchronous on the ctx stream.
 * The two workspaces are the caller's (slam_covis_workspace); the count workspace must live until slam_covis_pairs returns, the
 * pair workspace until slam_covis_edges has run.  Integers only; atomics only count, so every output is a function of the
 * input alone.  Limits: K <= SLAM_PG_MAX_VERTICES, L <= SLAM_BAS_MAX_POINTS, O <= SLAM_BAS_MAX_OBS, P <= SLAM_BAS_MAX_PAIRS,
 * E <= SLAM_PG_MAX_EDGES. */
/* h_limits [8] = {threads of a workgroup, keys of a sort tile, bits of a sort digit, entries of a scan tile, lanes ranked by one
 * ballot, the largest K with 32-bit pair keys, list lengths at which a kernel changes form (0: none), bytes of the scalar
 * block}; needs no device */
SLAM_API int slam_covis_limits(int32_t* h_limits);
/* h_plan [8] = {bits, passes, key bytes and tiles of the observation sort; bits, passes, key bytes and tiles of the pair sort
 * (P = 0: what is known without it)}; needs no device */
SLAM_API int slam_covis_plan(int64_t K, int64_t L, int64_t O, int64_t P, int32_t* h_plan);
/* h_bytes [2] = {the count workspace, the pair workspace for P pairs}; needs no device */
SLAM_API int slam_covis_workspace(int64_t K, int64_t L, int64_t O, int64_t P, uint64_t* h_bytes);
SLAM_API int slam_covis_count(slam_ctx* ctx, int64_t K, int64_t L, int64_t O, const int32_t* d_obs_pose, const int32_t* d_obs_point,
                              const uint8_t* d_fixed, void* d_count_ws, int64_t* h_scalars);
SLAM_API int slam_covis_pairs(slam_ctx* ctx, int64_t K, int64_t L, int64_t O, int64_t P, const void* d_count_ws, void* d_pair_ws,
                              int32_t* d_pair_a, int32_t* d_pair_b, int64_t* h_edges);
SLAM_API int slam_covis_edges(slam_ctx* ctx, int64_t K, int64_t P, int64_t E, const void* d_pair_ws, int32_t* d_edges, int32_t* d_weights,
                              int32_t* d_pair_ptr);
/* the observation table of slam_fuse_* (d_offsets int64 [M+1] ON THE DEVICE, d_obs int32 [nnz,2]) as d_obs_pose / d_obs_point
 * int32 [nnz]: slot s holds (frame of s, point whose list s lies in), so the pairs of slam_covis_pairs are slots of d_obs.
 * d_offsets must ascend from 0 to nnz.  Asynchronous on the ctx stream. */
SLAM_API int slam_covis_rows(slam_ctx* ctx, int64_t M, int64_t nnz, const int64_t* d_offsets, const int32_t* d_obs, int32_t* d_obs_pose,
                             int32_t* d_obs_point);

/* ---- local-map selection and keyframe culling (local_map.hip) -------------------------------------------------
 * Tracking::UpdateLocalKeyFrames' vote, UpdateLocalPoints and LocalMapping::KeyFrameCulling over tables that stay on the device
 * (the reference keeps a sliding window and no observation counts).  The map, as slam_fuse_* and slam_covis_rows take it:
 *   d_offsets int64 [M+1] ON THE DEVICE and d_obs int32 [nnz,2] = (frame, row), lists of at most 256 entries;
 *   d_frame_offsets int64 [F+1] ON THE DEVICE (h_frame_offsets: the same table on the host), n_rows = frame_offsets[F];
 *   d_frame_points int32 [n_rows] in row order (-1: none) and d_level int32 [n_rows] in row order;
 *   byte masks, each may be null: d_frame_removed [F] (a removed keyframe observes nothing, gets no vote, gives no local point
 *   and counts (0, 0) as a candidate) and d_point_bad [M] (a bad point takes no part anywhere).
 * Integers only.  Atomics count, or, and, or take a maximum, so every output is a function of the input alone.  No index outside
 * its range is dereferenced; what is met out of range is skipped and counted in slam_index_errors.  The workspaces are the
 * caller's (slam_lmap_workspace).  Limits: B <= 65535, F <= 2^24, M <= 2^24, nnz and n_rows < 2^31. */
/* h_limits [8] = {threads of a workgroup; frames whose vote counters take 16 KiB of LDS; frames whose vote counters fit the LDS
 * of a CU - above, the counters are global memory; the three lane-group sizes of slam_lmap_cull_count = the longest list each
 * takes in one step (16, 64, 256); bitmap words of a scan tile; bytes of the scalar block}; needs no device */
SLAM_API int slam_lmap_limits(int32_t* h_limits);
/* h_bytes [4] = {the workspace of slam_lmap_frame_points, of slam_lmap_vote for B queries, of slam_lmap_points_mark / _fill for B
 * queries over M points, of slam_lmap_cull_count for C candidates}; needs no device */
SLAM_API int slam_lmap_workspace(int64_t B, int64_t F, int64_t M, int64_t C, uint64_t* h_bytes);
/* The inverse table: d_frame_points = -1, then [frame_offsets[f] + r] = m for every slot (f, r) of point m.  Waits, and returns
 * h_scalars [2] = {slots whose frame or row is out of range (never dereferenced), claims of a row that already had a point}.
 * With a row claimed twice the table holds the greatest claimant and must not be used. */
SLAM_API int slam_lmap_frame_points(slam_ctx* ctx, int64_t M, int64_t nnz, const int64_t* d_offsets, const int32_t* d_obs, int64_t F,
                                    const int64_t* d_frame_offsets, int64_t n_rows, int32_t* d_frame_points, void* d_ws, int64_t* h_scalars);
/* The vote of B query frames: query b tracks the map points d_qpoints [h_qoffsets[b], h_qoffsets[b+1]) (-1 and bad points are
 * skipped; other entries outside [0, M) are skipped and counted).  d_votes int32 [B,F]: for every occurrence of a point in the
 * list, +1 for every frame of its observation list that is not removed.  d_best int32 [B,2] = (the frame with the most votes, the
 * lowest on ties; its votes) or (-1, 0); d_nvoted int32 [B] frames with a vote.  form: 0 = by F, 1 / 2 = the counters of a
 * query in 16 KiB / all the LDS of a CU (F must fit), 3 = in global memory; every form gives the same bytes.  h_skipped null:
 * asynchronous on the ctx stream; else waits and returns the entries counted. */
SLAM_API int slam_lmap_vote(slam_ctx* ctx, int64_t B, const int32_t* d_qpoints, const int64_t* h_qoffsets, int64_t M, int64_t nnz,
                            const int64_t* d_offsets, const int32_t* d_obs, const uint8_t* d_point_bad, int64_t F, const uint8_t* d_frame_removed,
                            int form, void* d_ws, int32_t* d_votes, int32_t* d_best, int32_t* d_nvoted, int64_t* h_skipped);
/* The local points of B queries in two phases.  mark: d_bitmap uint32 [B, ceil(M / 32)] = 0, then bit m of row b is set for
 * every row of the frames d_lkf [h_lkf_offsets[b], h_lkf_offsets[b+1]) that holds a point m that is not bad (a removed frame
 * has no rows), then cleared for every point of the query's own list d_qpoints; waits, and returns h_counts int64 [B], the bits
 * set per query.  fill: writes the points of query b, ascending, to d_lpoints [h_out_offsets[b], ...) and never past
 * h_out_offsets[b+1]; asynchronous on the ctx stream.  The workspace and the bitmap must live from mark until fill has run. */
SLAM_API int slam_lmap_points_mark(slam_ctx* ctx, int64_t B, const int32_t* d_lkf, const int64_t* h_lkf_offsets, const int32_t* d_qpoints,
                                   const int64_t* h_qoffsets, int64_t M, const uint8_t* d_point_bad, int64_t F, const int64_t* d_frame_offsets,
                                   int64_t n_rows, const int32_t* d_frame_points, const uint8_t* d_frame_removed, uint32_t* d_bitmap, void* d_ws,
                                   int64_t* h_counts);
SLAM_API int slam_lmap_points_fill(slam_ctx* ctx, int64_t B, int64_t M, const uint32_t* d_bitmap, void* d_ws, const int64_t* h_out_offsets,
                                   int32_t* d_lpoints);
/* KeyFrameCulling's count for the C candidate frames h_cand (null: all F frames, C is ignored).  For a row r of candidate c that
 * holds a point m that is not bad, with N the observers of m that are not removed and l = d_level[r]: n_points += 1; if
 * N > th_obs and at least th_obs observers (f, r') with f != c have d_level[frame_offsets[f] + r'] <= l + 1, n_redundant += 1.
 * d_counts int32 [C,2] = (n_points, n_redundant), on 8 bytes; d_flags (may be null) u8 per candidate row, the candidates in
 * order: 0 no point, 1 counted, 2 redundant.  max_list: no list is longer (a lower value costs time, never a verdict).
 * C times the rows of the longest candidate must not exceed 2^24 (split the candidates).  Asynchronous on the ctx stream. */
SLAM_API int slam_lmap_cull_count(slam_ctx* ctx, int64_t C, const int32_t* h_cand, int64_t M, int64_t nnz, const int64_t* d_offsets,
                                  const int32_t* d_obs, const uint8_t* d_point_bad, int64_t F, const int64_t* h_frame_offsets,
                                  const int64_t* d_frame_offsets, const int32_t* d_frame_points, const int32_t* d_level,
                                  const uint8_t* d_frame_removed, int th_obs, int max_list, void* d_ws, int32_t* d_counts, uint8_t* d_flags);

/* ---- loop and relocalisation candidates (loop_detect.hip) ------------------------------------------------------
 * The covisibility-group stage of ORB-SLAM's KeyFrameDatabase::DetectLoopCandidates and DetectRelocalizationCandidates for Q
 * queries over E database entries (entry id = keyframe index), on tables that stay on the device.  The reference detects no
 * loops: there is no call site to compare with, PARITY UNPINNED (as for the bag-of-words database, 4j).
 *   d_s uint32 [Q,E] and d_common int32 [Q,E]: the dense form of slam_bow_query.
 *   d_best int32 [E,nb], 0 <= nb <= 16: row i = GetBestCovisibilityKeyFrames(nb) of keyframe i, padded with -1.  A negative
 *   entry is padding; an entry >= E in the row of a candidate is skipped and counted (slam_index_errors).  The table is the
 *   caller's: a row that repeats an id or names itself is summed as written.
 *   d_excl [h_excl_offsets[q] .. h_excl_offsets[q+1]): the excluded entries of query q - its connected keyframes and itself;
 *   ids outside [0, E) are skipped and counted.  h_own int32 [Q]: the query's own entry, -1 for a frame not in the database.
 *   h_limit int32 [Q], each in [0, E], or null (E for every query): entries with id >= limit are excluded as well, so that a
 *   trajectory can be replayed in one call, each keyframe seeing only its past.
 *   h_min_s uint32 [Q]: a threshold on s, or 0xFFFFFFFF = derive it: the least d_s[q,j] over the excluded j in [0, E) other
 *   than h_own[q], and 2^31 (a score of 1) when there is none - ORB-SLAM's minScore.  Null: derived for every query.
 *   mode 0 = loop; 1 = relocalisation: no excluded list, min_s = 0 (d_excl, h_excl_offsets, h_own and h_min_s are not read).
 * Per query q:
 *   1. shares(i): i is not excluded, i < limit and common[i] > 0.
 *   2. cmax = the maximum of common over those entries; words_ok(i): shares(i) and 5 common[i] > 4 cmax (for
 *      1 <= c <= cmax <= 8192 the same as ORB-SLAM's c > int(0.8f cmax)).
 *   3. i is a candidate when words_ok(i) and s[i] >= min_s.
 *   4. acc[i] (64 bits) = s[i] + the sum of s[j] over the j of d_best[i] with words_ok(j) - the word filter only, not min_s.
 *   5. gbest[i] = the entry of greatest s among i and those j; on ties the candidate itself, then the earlier position.
 *   6. acc_max = the maximum of acc over the candidates; candidate i is retained when 4 acc[i] > 3 acc_max.
 *   7. The result is the set {gbest[i] : i retained}: no duplicates, ascending by id, each member with its own s.
 * With cmax = 0 or no candidate the result is empty.  Integers only; atomics take a maximum, set bits or count, so two runs
 * give the same bytes.  The workspace is the caller's.  Limits: Q <= 65535, 1 <= E <= 2^24. */
/* h_limits [4] = {threads of a workgroup, entries of a tile over E, the largest nb, the largest Q}; needs no device */
SLAM_API int slam_loop_limits(int32_t* h_limits);
/* *h_bytes = the workspace of slam_loop_candidates / slam_loop_fill for Q queries over E entries (the excluded lists are the
 * caller's d_excl); needs no device */
SLAM_API int slam_loop_workspace(int64_t Q, int64_t E, uint64_t* h_bytes);
/* Steps 1 - 6 and the mark of step 7: d_acc uint64 [Q,E] and d_gbest int32 [Q,E] (0 and -1 where i is no candidate), d_bitmap
 * uint32 [Q, ceil(E / 32)] the result set.  Waits, and returns h_counts int64 [Q], the members per query, and *h_skipped (may
 * be null), the ids this call skipped and counted. */
SLAM_API int slam_loop_candidates(slam_ctx* ctx, int64_t Q, int64_t E, const uint32_t* d_s, const int32_t* d_common, int nb, const int32_t* d_best,
                                  const int32_t* d_excl, const int64_t* h_excl_offsets, const int32_t* h_own, const int32_t* h_limit,
                                  const uint32_t* h_min_s, int mode, void* d_ws, uint64_t* d_acc, int32_t* d_gbest, uint32_t* d_bitmap,
                                  int64_t* h_counts, int64_t* h_skipped);
/* The fill of step 7: the members of query q, ascending, to d_ids [h_out_offsets[q], ...) and their s to d_scores, never past
 * h_out_offsets[q+1]; asynchronous on the ctx stream.  The workspace and the bitmap must live from slam_loop_candidates until
 * the fill has run. */
SLAM_API int slam_loop_fill(slam_ctx* ctx, int64_t Q, int64_t E, const uint32_t* d_s, const uint32_t* d_bitmap, void* d_ws,
                            const int64_t* h_out_offsets, int32_t* d_ids, uint32_t* d_scores);

/* ---- multi-GPU: RCCL all-gather of per-shard result rows ---------------- */
#define SLAM_COMM_ID_BYTES 128
SLAM_API int slam_comm_version(int* version); /* ncclGetVersion of the librccl that was loaded (e.g. 22703); needs no GPU */
SLAM_API int slam_comm_unique_id(void* h_id /*[128]*/);
SLAM_API int slam_comm_init(slam_ctx* ctx, int nranks, int rank, const void* h_id);
SLAM_API int slam_comm_destroy(slam_ctx* ctx);
/* every rank contributes bytes_per_rank bytes; d_recv holds nranks*bytes_per_rank.
 * in-place allowed when d_send == d_recv + rank*bytes_per_rank. */
SLAM_API int slam_comm_allgather(slam_ctx* ctx, const void* d_send, void* d_recv, uint64_t bytes_per_rank);
SLAM_API int slam_comm_broadcast(slam_ctx* ctx, void* d_buf, uint64_t bytes, int root);
/* Double-buffered form for back-to-back passes: the all-gather of result buffer `buffer_id` (0 or 1) runs on a
 * second stream of the ctx, ordered after everything issued so far on the main stream, so the next pass (which
 * writes the OTHER buffer) overlaps it.  slam_comm_wait_buffer makes the main stream wait until the last
 * gather of that buffer has finished (call it before overwriting the buffer); slam_sync waits for both streams. */
SLAM_API int slam_comm_allgather_overlapped(slam_ctx* ctx, const void* d_send, void* d_recv, uint64_t bytes_per_rank,
                                            int buffer_id);
SLAM_API int slam_comm_wait_buffer(slam_ctx* ctx, int buffer_id);

/* ---- multi-GPU without a communicator library: direct all-gather over xGMI peer mappings (HIP IPC) ----
 * Each rank exports its gathered buffer(s) (slam_p2p_export on the base pointer of a slam_malloc allocation),
 * the launcher ships the 64-byte handles around, every rank maps the peers' buffers (slam_p2p_open) and
 * slam_p2p_allgather_overlapped then copies this rank's slot (bytes_per_rank at offset rank*bytes_per_rank) into
 * every peer's buffer on the context's second stream, behind the work queued so far on the main stream.
 * h_peer_bufs is a HOST array of nranks device pointers (entry [rank] unused).  slam_comm_wait_buffer(buffer_id)
 * orders later main-stream work after these copies; arrival on the peers is the launcher's barrier to guarantee.
 * No reference counterpart (the reference is single-process). */
#define SLAM_P2P_HANDLE_BYTES 64
SLAM_API int slam_p2p_export(slam_ctx* ctx, void* d_ptr, void* h_handle /*[64]*/);
SLAM_API int slam_p2p_open(slam_ctx* ctx, const void* h_handle, void** d_peer_ptr);
SLAM_API int slam_p2p_close(slam_ctx* ctx, void* d_peer_ptr);
SLAM_API int slam_p2p_allgather_overlapped(slam_ctx* ctx, const void* d_send, uint64_t bytes_per_rank, int rank,
                                           void* const* h_peer_bufs, int nranks, int buffer_id);

#ifdef __cplusplus
}
#endif
#endif /* SLAMHIP_H */
