"""ctypes binding of libslamhip.so (the C ABI declared in include/slamhip.h).

The product path has no CPU fallback: if the shared library is missing or no
gfx950 device is visible, every entry point raises.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_uint8, c_uint64, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(os.path.dirname(_HERE), "lib", "libslamhip.so")

SLAM_OK = 0
NO_MATCH_IDX = -1
NO_MATCH_DIST = 2**31 - 1
DESC_BYTES = 32
COMM_ID_BYTES = 128
P2P_HANDLE_BYTES = 64


class SlamHipError(RuntimeError):
    """A libslamhip call returned a negative status."""

    def __init__(self, code: int, message: str):
        super().__init__(f"libslamhip error {code}: {message}")
        self.code = code


class SlamHipBusy(SlamHipError):
    """SLAM_ERR_BUSY (-6): a resource condition, not a caller error - a kernel that needs all its workgroups resident at once
    could not get them (other work holds compute units).  Inputs and outputs are untouched; retry, or use the form without
    a residency requirement."""


SLAM_ERR_INVALID, SLAM_ERR_BUSY = -1, -6


# name -> (restype, argtypes); must list every SLAM_API symbol of include/slamhip.h
SIGNATURES = {
    "slam_last_error": (c_char_p, []),
    "slam_version": (c_char_p, []),
    "slam_device_count": (c_int, [POINTER(c_int)]),
    "slam_ctx_create": (c_int, [c_int, POINTER(c_void_p)]),
    "slam_ctx_destroy": (c_int, [c_void_p]),
    "slam_ctx_device": (c_int, [c_void_p, POINTER(c_int)]),
    "slam_sync": (c_int, [c_void_p]),
    "slam_malloc": (c_int, [c_void_p, c_uint64, POINTER(c_void_p)]),
    "slam_free": (c_int, [c_void_p, c_void_p]),
    "slam_memset": (c_int, [c_void_p, c_void_p, c_int, c_uint64]),
    "slam_copy": (c_int, [c_void_p, c_void_p, c_void_p, c_uint64]),
    "slam_upload": (c_int, [c_void_p, c_void_p, c_void_p, c_uint64]),
    "slam_download": (c_int, [c_void_p, c_void_p, c_void_p, c_uint64]),
    "slam_timer_start": (c_int, [c_void_p]),
    "slam_timer_stop": (c_int, [c_void_p, POINTER(c_float)]),
    "slam_prof_enable": (c_int, [c_void_p, c_int]),
    "slam_prof_read": (c_int, [c_void_p, POINTER(c_int64), POINTER(c_double)]),
    "slam_bf_knn2_u256": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int64, c_void_p, c_void_p]),
    "slam_bf_knn2_batch_u256": (c_int, [c_void_p, c_int64, c_void_p]),
    "slam_bf_knn2_select_u256": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_int, c_double,
                                         c_void_p, POINTER(c_int64)]),
    "slam_bf_merge_top2": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p]),
    "slam_bf_knn2_u256_host": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p]),
    "slam_bf_knn_u256": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int64, c_int, c_void_p, c_void_p]),
    "slam_bf_knn_u256_host": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int, c_void_p, c_void_p]),
    "slam_bf_merge_topk": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int, c_void_p, c_void_p]),
    "slam_bf_topk_plan_describe": (c_int, [c_int, c_int64, c_int64, c_int, POINTER(c_int32)]),
    "slam_bf_radius_u256": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_float, c_int64, c_void_p, c_int64, c_void_p,
                                    c_void_p, POINTER(c_int64)]),
    "slam_bf_radius_u256_host": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_float, c_void_p, c_int64, c_void_p,
                                         c_void_p, POINTER(c_int64)]),
    "slam_bf_radius_threshold": (c_int, [c_float]),
    "slam_bf_radius_plan_describe": (c_int, [c_int, c_int64, c_int64, POINTER(c_int32)]),
    "slam_bf_window_knn_u256": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_float,
                                        c_int, c_int64, c_void_p, c_void_p]),
    "slam_bf_window_knn_u256_host": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p,
                                             c_float, c_int, c_int64, c_void_p, c_void_p]),
    "slam_bf_window_plan_describe": (c_int, [c_int, c_int64, c_int64, c_int64, POINTER(c_int64)]),
    "slam_bf_set_tuning": (c_int, [c_void_p, POINTER(c_int32), c_int]),
    "slam_bf_plan_info": (c_int, [c_void_p, c_int64, c_int64, POINTER(c_int32)]),
    "slam_bf_plan_describe": (c_int, [c_int, POINTER(c_int32), c_int, c_int64, c_int64, c_int64, c_int, POINTER(c_int32),
                                      POINTER(c_int32), c_int64, POINTER(c_int64)]),
    "slam_bf_set_engine": (c_int, [c_void_p, c_int]),
    "slam_bf_mx_plan_describe": (c_int, [c_int, c_int64, c_int64, POINTER(c_int32), POINTER(c_int32), c_int64, POINTER(c_int64)]),
    "slam_bf_mx_tile_describe": (c_int, [c_int, c_int64, c_int64, POINTER(c_int32)]),
    "slam_bf_set_mx_feed": (c_int, [c_void_p, c_int]),
    "slam_bf_mx_feed_describe": (c_int, [c_int, c_int64, c_int64, POINTER(c_int32)]),
    "slam_bf_mx_image_bytes": (c_int, [c_void_p, POINTER(c_int64)]),
    "slam_bf_mx_image_fill": (c_int, [c_void_p, c_int]),
    "slam_bf_train_pin": (c_int, [c_void_p, c_void_p, c_int64]),
    "slam_bf_train_refresh": (c_int, [c_void_p, c_void_p]),
    "slam_bf_train_unpin": (c_int, [c_void_p, c_void_p]),
    "slam_bf_mx_feed_describe_pinned": (c_int, [c_int, c_int64, c_int64, POINTER(c_int32)]),
    "slam_bf_mx_image_launches": (c_int, [c_void_p, POINTER(c_int64)]),
    "slam_bf_train_pins": (c_int, [c_void_p, POINTER(c_int64)]),
    "slam_bf_reset_state": (c_int, [c_void_p]),
    "slam_bf_state_dirty": (c_int, [c_void_p, POINTER(c_int64)]),
    "slam_bf_match_filter": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int, c_double, c_void_p,
                                     POINTER(c_int64), POINTER(c_int32)]),
    "slam_bf_cross_check": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p,
                                    POINTER(c_int64)]),
    "slam_bf_split_index": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p]),
    "slam_reproj_rj_f64": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p,
                                   c_int64, c_double, c_double, c_double, c_double, c_void_p, c_void_p, c_void_p]),
    "slam_pose_normal_eq_f64": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_double,
                                        c_double, c_double, c_double, c_double, c_void_p, c_void_p, c_void_p]),
    "slam_pose_optimize_f64": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_double, c_double, c_double,
                                       c_double, c_int, c_int, c_double, c_double, c_void_p, c_void_p, c_void_p,
                                       c_void_p]),
    "slam_pose_optimize_batch_f64": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_double,
                                             c_double, c_double, c_double, c_int, c_int, c_double, c_double, c_void_p,
                                             c_void_p, c_void_p, c_void_p]),
    "slam_tv_fivepoint_f64": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p]),
    "slam_tv_essential_ransac_f64": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_double, c_double, c_double,
                                             c_double, c_int, c_double, c_uint64, c_void_p, c_void_p, c_void_p]),
    "slam_tv_recover_pose_f64": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_double, c_double, c_double,
                                         c_double, c_void_p, c_void_p, c_double, c_void_p, c_void_p, c_void_p]),
    "slam_tv_triangulate_f64": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "slam_pnp_p3p_f64": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p]),
    "slam_pnp_ransac_f64": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_double, c_double, c_double, c_double,
                                    c_int, c_double, c_uint64, c_void_p, c_void_p, c_void_p]),
    "slam_hg_fourpoint_f64": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p]),
    "slam_hg_ransac_f64": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_double, c_uint64, c_void_p,
                                   c_void_p, c_void_p]),
    "slam_hg_decompose_f64": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_double, c_double, c_double, c_double,
                                      c_void_p, c_void_p, c_double, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                      c_void_p]),
    "slam_hg_model_score_f64": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_double, c_double, c_double,
                                        c_double, c_void_p, c_void_p, c_double, c_void_p, c_void_p]),
    "slam_sim3_threepoint_f64": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    "slam_sim3_ransac_f64": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_double, c_double, c_double,
                                     c_double, c_int, c_double, c_int, c_uint64, c_void_p, c_void_p, c_void_p]),
    "slam_sim3_refit_f64": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int, c_void_p, c_void_p]),
    "slam_sim3_optimize_f64": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p,
                                       c_double, c_double, c_double, c_double, c_double, c_int, c_int, c_int, c_int, c_int, c_void_p,
                                       c_void_p, c_void_p, c_void_p]),
    "slam_cam_undistort_f64": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "slam_cam_distort_f64": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "slam_cam_rectify_map": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p]),
    "slam_cam_remap_u8": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_int64, c_int64, c_int64, c_void_p, c_int64, c_int64, c_int, c_void_p,
                                  c_int64, c_int64, c_void_p]),
    "slam_stereo_workspace": (c_int, [c_int64, c_int64, POINTER(c_uint64)]),
    "slam_stereo_match": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p,
                                  c_void_p, c_int64, c_int, c_uint64, c_uint64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_double, c_double,
                                  c_double, c_int, c_int, c_int, c_int, c_void_p, c_uint64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                  c_void_p]),
    "slam_pg_workspace": (c_int, [c_int64, c_int64, POINTER(c_uint64)]),
    "slam_pg_plan": (c_int, [c_int64, c_int64, POINTER(c_int32)]),
    "slam_pg_linearize_f64": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                      c_double, c_void_p, c_void_p, c_void_p, c_void_p, POINTER(c_int32)]),
    "slam_pg_hmul_f64": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                 c_double, c_void_p, c_void_p]),
    "slam_pg_pcg_f64": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                c_void_p, c_double, c_double, c_int, c_void_p, c_void_p]),
    "slam_pg_optimize_f64": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64,
                                     c_void_p, c_void_p, c_int, c_double, c_double, c_int, c_void_p, c_void_p]),
    "slam_pg_optimize_host_f64": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                                          c_double, c_double, c_int, c_void_p, c_void_p]),
    "slam_s3g_workspace": (c_int, [c_int64, c_int64, POINTER(c_uint64)]),
    "slam_s3g_plan": (c_int, [c_int64, c_int64, POINTER(c_int32)]),
    "slam_s3g_linearize_f64": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                       c_double, c_void_p, c_void_p, c_void_p, c_void_p, POINTER(c_int32)]),
    "slam_s3g_hmul_f64": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                  c_double, c_void_p, c_void_p]),
    "slam_s3g_pcg_f64": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                 c_void_p, c_double, c_double, c_int, c_void_p, c_void_p]),
    "slam_s3g_optimize_f64": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64,
                                      c_void_p, c_void_p, c_int, c_double, c_double, c_int, c_int, c_void_p, c_void_p]),
    "slam_s3g_optimize_host_f64": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                                           c_double, c_double, c_int, c_int, c_void_p, c_void_p]),
    "slam_orb_workspace": (c_int, [c_int64, c_int64, c_int64, c_int, c_void_p, c_void_p, c_int64, POINTER(c_uint64), c_void_p]),
    "slam_orb_extract_u8": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_int64, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                    c_int, c_void_p, c_void_p, c_uint64, c_void_p, c_void_p, c_void_p, c_void_p]),
    "slam_orb_dist_workspace": (c_int, [c_int64, c_int64, c_int64, c_int, c_void_p, c_void_p, c_void_p, POINTER(c_uint64), c_void_p]),
    "slam_orb_extract_dist_u8": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_int64, c_void_p, c_int, c_int, c_void_p, c_void_p,
                                         c_void_p, c_int, c_int, c_void_p, c_void_p, c_uint64, c_void_p, c_void_p, c_void_p, c_void_p]),
    "slam_orb_extract_u8_host": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_int64, c_void_p, c_int, c_int, c_void_p, c_void_p,
                                         c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "slam_bf_match_host": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_int, c_double,
                                   c_void_p, c_void_p, c_void_p, c_void_p]),
    "slam_index_errors": (c_int, [c_void_p, POINTER(c_int64)]),
    "slam_io_counters": (c_int, [c_void_p, POINTER(c_uint64), POINTER(c_uint64)]),
    "slam_ctx_block_bytes": (c_int, [c_void_p, POINTER(c_int64), c_int]),
    "slam_ctx_block_fill": (c_int, [c_void_p, c_int, c_int]),
    "slam_pose_optimize_host_f64": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_double, c_double,
                                            c_double, c_double, c_int, c_int, c_double, c_double, c_void_p, c_void_p,
                                            c_void_p, c_void_p]),
    "slam_ba_reduce_f64": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p,
                                   c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_double, c_double,
                                   c_double, c_double, c_double, c_double, c_void_p, c_void_p, c_void_p, c_void_p,
                                   c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "slam_ba_cost_f64": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_double,
                                 c_double, c_double, c_double, c_double, c_void_p]),
    "slam_ba_backsub_f64": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                    c_void_p, c_void_p]),
    "slam_ba_optimize_workspace": (c_int, [c_int64, c_int64, c_int64, POINTER(c_uint64)]),
    "slam_ba_optimize_shape": (c_int, [c_int64, c_int64, c_int64, POINTER(c_int32), POINTER(c_int32)]),
    "slam_ba_optimize_host_f64": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                          c_void_p, c_double, c_double, c_double, c_double, c_double, c_int, c_void_p, c_void_p,
                                          c_void_p]),
    "slam_ba_optimize_f64": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                     c_void_p, c_void_p, c_int64, c_double, c_double, c_double, c_double, c_double, c_int, c_void_p,
                                     c_void_p, c_void_p, c_uint64, c_void_p]),
    "slam_bas_workspace": (c_int, [c_int64, c_int64, c_int64, c_int64, c_int64, POINTER(c_uint64)]),
    "slam_bas_plan": (c_int, [c_int64, c_int64, c_int64, c_int64, c_int64, POINTER(c_int32)]),
    "slam_bas_linearize_f64": (c_int, [c_void_p, c_int64, c_int64, c_int64] + [c_void_p] * 10 + [c_double] * 5 + [c_void_p] * 7),
    "slam_bas_cost_f64": (c_int, [c_void_p, c_int64, c_int64, c_int64] + [c_void_p] * 7 + [c_double] * 5 + [c_void_p] * 2),
    "slam_bas_reduce_f64": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_int64, c_int64] + [c_void_p] * 12 + [c_double] + [c_void_p] * 5),
    "slam_bas_backsub_f64": (c_int, [c_void_p, c_int64, c_int64, c_int64] + [c_void_p] * 8),
    "slam_bas_candidate_f64": (c_int, [c_void_p, c_int64, c_int64] + [c_void_p] * 7 + [c_double] + [c_void_p] * 4),
    "slam_bas_linearize_stereo_f64": (c_int, [c_void_p, c_int64, c_int64, c_int64] + [c_void_p] * 11 + [c_double] * 7 + [c_void_p] * 7),
    "slam_bas_cost_stereo_f64": (c_int, [c_void_p, c_int64, c_int64, c_int64] + [c_void_p] * 8 + [c_double] * 7 + [c_void_p] * 2),
    "slam_bas_classify_stereo_f64": (c_int, [c_void_p, c_int64, c_int64, c_int64] + [c_void_p] * 6 + [c_double] * 7 + [c_void_p] * 2),
    "slam_reproj_rj_stereo_f64": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_int64]
                                + [c_double] * 7 + [c_void_p] * 5),
    "slam_pose_optimize_stereo_batch_f64": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64]
                                            + [c_double] * 5 + [c_int, c_int] + [c_double] * 4 + [c_void_p] * 4),
    "slam_bow_limits": (c_int, [POINTER(c_int32)]),
    "slam_bow_transform": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_int, c_void_p, c_void_p]),
    "slam_bow_vectors": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_int64, c_void_p, c_uint64, c_void_p,
                                 c_void_p, c_void_p, c_void_p]),
    "slam_bow_vectors_workspace": (c_int, [c_int64, c_int64, POINTER(c_uint64)]),
    "slam_bow_group_keys": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p]),
    "slam_bow_index_build": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p]),
    "slam_bow_query": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_int,
                               c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "slam_bow_train_seed": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int, c_void_p, c_void_p, c_void_p, c_uint64]),
    "slam_bow_train_seed_workspace": (c_int, [c_int64, c_int64, POINTER(c_uint64)]),
    "slam_bow_train_step": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int64,
                                    c_void_p, c_void_p, c_void_p, c_int, POINTER(c_int64)]),
    "slam_bow_train_descend": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int, c_void_p, c_void_p]),
    "slam_bow_match_limits": (c_int, [POINTER(c_int32)]),
    "slam_bow_match_plan_describe": (c_int, [c_int64, c_int64, POINTER(c_int64)]),
    "slam_bow_match_group": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p]),
    "slam_bow_match_top2": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_void_p, c_void_p]),
    "slam_bow_match_search": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_double, c_int, c_void_p, c_void_p,
                                      c_void_p, c_void_p]),
    "slam_proj_match_limits": (c_int, [POINTER(c_int32)]),
    "slam_proj_match_plan_describe": (c_int, [c_int64, c_int64, c_int64, POINTER(c_int64)]),
    "slam_proj_match_grid": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_int, c_void_p,
                                     c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "slam_proj_match_project": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p,
                                        c_void_p, c_void_p]),
    "slam_proj_match_search": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p,
                                       c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "slam_tri_match_limits": (c_int, [POINTER(c_int32)]),
    "slam_tri_match_plan_describe": (c_int, [c_int64, c_int64, POINTER(c_int64)]),
    "slam_tri_match_search": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p,
                                      c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "slam_tri_match_triangulate": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64,
                                           c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                           c_void_p, c_void_p]),
    "slam_fuse_limits": (c_int, [POINTER(c_int32)]),
    "slam_fuse_search": (c_int, [c_void_p] * 8 + [c_int64] + [c_void_p] * 4 + [c_int64] + [c_void_p] * 10),
    "slam_fuse_refresh": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p,
                                  c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int] + [c_void_p] * 4),
    "slam_covis_limits": (c_int, [POINTER(c_int32)]),
    "slam_covis_plan": (c_int, [c_int64, c_int64, c_int64, c_int64, POINTER(c_int32)]),
    "slam_covis_workspace": (c_int, [c_int64, c_int64, c_int64, c_int64, POINTER(c_uint64)]),
    "slam_covis_count": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, POINTER(c_int64)]),
    "slam_covis_pairs": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, POINTER(c_int64)]),
    "slam_covis_edges": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p]),
    "slam_covis_rows": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p]),
    "slam_lmap_limits": (c_int, [POINTER(c_int32)]),
    "slam_lmap_workspace": (c_int, [c_int64, c_int64, c_int64, c_int64, POINTER(c_uint64)]),
    "slam_lmap_frame_points": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p,
                                       POINTER(c_int64)]),
    "slam_lmap_vote": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int,
                               c_void_p, c_void_p, c_void_p, c_void_p, POINTER(c_int64)]),
    "slam_lmap_points_mark": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64,
                                      c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "slam_lmap_points_fill": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p]),
    "slam_lmap_cull_count": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p,
                                     c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "slam_loop_limits": (c_int, [POINTER(c_int32)]),
    "slam_loop_workspace": (c_int, [c_int64, c_int64, POINTER(c_uint64)]),
    "slam_loop_candidates": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                     c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, POINTER(c_int64)]),
    "slam_loop_fill": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "slam_comm_version": (c_int, [POINTER(c_int)]),
    "slam_comm_unique_id": (c_int, [c_void_p]),
    "slam_comm_init": (c_int, [c_void_p, c_int, c_int, c_void_p]),
    "slam_comm_destroy": (c_int, [c_void_p]),
    "slam_comm_allgather": (c_int, [c_void_p, c_void_p, c_void_p, c_uint64]),
    "slam_comm_broadcast": (c_int, [c_void_p, c_void_p, c_uint64, c_int]),
    "slam_comm_allgather_overlapped": (c_int, [c_void_p, c_void_p, c_void_p, c_uint64, c_int]),
    "slam_comm_wait_buffer": (c_int, [c_void_p, c_int]),
    "slam_p2p_export": (c_int, [c_void_p, c_void_p, c_void_p]),
    "slam_p2p_open": (c_int, [c_void_p, c_void_p, POINTER(c_void_p)]),
    "slam_p2p_close": (c_int, [c_void_p, c_void_p]),
    "slam_p2p_allgather_overlapped": (c_int, [c_void_p, c_void_p, c_uint64, c_int, c_void_p, c_int, c_int]),
}

class BfSearch(ctypes.Structure):
    """``slam_bf_search`` of include/slamhip.h: one entry of a batched search."""

    _fields_ = [("d_query", c_void_p), ("N", c_int64), ("d_train", c_void_p), ("M", c_int64), ("train_base", c_int64),
                ("d_idx", c_void_p), ("d_dist", c_void_p)]


class BowGroups(ctypes.Structure):
    """``slam_bow_groups`` of include/slamhip.h: one set of grouped images."""

    _fields_ = [("d_desc", c_void_p), ("d_nodes", c_void_p), ("d_order", c_void_p), ("d_inverse", c_void_p), ("d_bins", c_void_p),
                ("h_offsets", c_void_p), ("B", c_int64)]


class ProjFrames(ctypes.Structure):
    """``slam_proj_frames`` of include/slamhip.h: one set of frames in grid order."""

    _fields_ = [("d_desc", c_void_p), ("d_cells", c_void_p), ("d_order", c_void_p), ("d_xy", c_void_p), ("d_meta", c_void_p),
                ("d_level", c_void_p), ("d_bins", c_void_p), ("h_offsets", c_void_p), ("B", c_int64), ("W", c_int32), ("H", c_int32),
                ("cell", c_int32), ("pad", c_int32)]


class ProjPoints(ctypes.Structure):
    """``slam_proj_points`` of include/slamhip.h: sets of map points."""

    _fields_ = [("d_xyz", c_void_p), ("d_desc", c_void_p), ("d_range", c_void_p), ("d_normal", c_void_p), ("d_level", c_void_p),
                ("d_bins", c_void_p), ("h_offsets", c_void_p), ("B", c_int64)]


class ProjParams(ctypes.Structure):
    """``slam_proj_params`` of include/slamhip.h: camera, bounds, scale tables and rules of one projection search."""

    _fields_ = [("fx", c_double), ("fy", c_double), ("cx", c_double), ("cy", c_double), ("min_x", c_double), ("max_x", c_double),
                ("min_y", c_double), ("max_y", c_double), ("cos2_limit", c_double), ("ratio", c_double), ("h_scale", c_void_p),
                ("h_scale2", c_void_p), ("n_levels", c_int32), ("th_high", c_int32), ("level_rule", c_int32), ("lo", c_int32), ("hi", c_int32),
                ("pad", c_int32)]


class TriViews(ctypes.Structure):
    """``slam_tri_views`` of include/slamhip.h: pixels, levels and taken marks of a set's rows."""

    _fields_ = [("d_xy", c_void_p), ("d_level", c_void_p), ("d_taken", c_void_p)]


class TriParams(ctypes.Structure):
    """``slam_tri_params`` of include/slamhip.h: camera, gates and level tables of the epipolar search and the triangulation."""

    _fields_ = [("fx", c_double), ("fy", c_double), ("cx", c_double), ("cy", c_double), ("chi2", c_double), ("epipole_r2", c_double),
                ("cos_max", c_double), ("chi2_px", c_double), ("ratio_factor", c_double), ("h_scale", c_void_p), ("h_sigma2", c_void_p),
                ("n_levels", c_int32), ("th_low", c_int32)]


class FuseParams(ctypes.Structure):
    """``slam_fuse_params`` of include/slamhip.h: the margins, the chi-square bound and the distance bound of one fusion search."""

    _fields_ = [("m_lo2", c_double), ("m_hi2", c_double), ("chi2", c_double), ("th_low", c_int32), ("pad", c_int32)]


BF_BATCH_MAX = 32
BF_KNN_MAX = 32             # SLAM_BF_KNN_MAX: the largest k of the top-k search
_lib = None


def load() -> ctypes.CDLL:
    """Load libslamhip.so and attach the signatures; raises if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(make -C slam-experiments_amd/csrc). There is no CPU fallback."
        )
    lib = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the ABI and this table disagree
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def addr(a) -> int:
    """Address of a C-contiguous numpy array: 0.46 us through the buffer protocol against 1.3-1.4 us for ``a.ctypes.data`` or
    ``a.__array_interface__`` (a frame-sized ``match()`` is a 5 us kernel; the per-frame host calls pass up to nine pointers)."""
    try:
        return ctypes.addressof(ctypes.c_char.from_buffer(a))
    except (TypeError, ValueError):              # a read-only or empty array has no writable buffer to borrow
        return a.__array_interface__["data"][0]


def check(rc: int) -> None:
    if rc != SLAM_OK:
        msg = load().slam_last_error()
        raise (SlamHipBusy if rc == SLAM_ERR_BUSY else SlamHipError)(rc, msg.decode("utf-8", "replace") if msg else "unknown error")


def device_count() -> int:
    n = c_int(0)
    rc = load().slam_device_count(ctypes.byref(n))
    return n.value if rc == SLAM_OK else 0
