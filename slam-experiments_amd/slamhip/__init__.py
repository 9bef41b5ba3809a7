"""slamhip — MI355X (gfx950) kernels for the descriptor-matching / reprojection
hot path of ViV99/slam-experiments, behind a ctypes C ABI (include/slamhip.h)."""
from ._lib import NO_MATCH_DIST, NO_MATCH_IDX, SlamHipBusy, SlamHipError, device_count, load  # noqa: F401
from .device import Context, DeviceBuffer, default_context, mx_feed_describe, mx_feed_describe_pinned, mx_plan_describe, mx_tile_describe, plan_describe  # noqa: F401
from .matching import (  # noqa: F401
    NORM_HAMMING,
    DeviceDescriptors,
    KeyframeDatabase,
    ResidentMatcher,
    Top2Table,
    as_descriptors,
    check_topk_k,
    cross_check_arrays,
    knn2_device,
    knn2_device_batch,
    knn2_select_device,
    knn_match_arrays,
    knn_match_arrays_batch,
    knn_match_collection,
    knn_topk_device,
    match_arrays,
    plan_describe_radius,
    plan_describe_topk,
    plan_describe_window,
    radius_device,
    radius_match_arrays,
    radius_match_collection,
    radius_threshold,
    ratio_test_arrays,
    split_image_index,
    topk_match_arrays,
    topk_match_collection,
    window_knn_device,
    window_match_arrays,
    window_match_filtered,
)
from .homography import (  # noqa: F401
    decompose_homography_arrays,
    decompose_homography_batch,
    decompose_homography_offsets,
    estimate_two_view_auto,
    find_homography_arrays,
    find_homography_batch,
    find_homography_offsets,
    fourpoint_homography_arrays,
    model_scores_offsets,
    verify_pairs_auto,
)
from .orb import (  # noqa: F401
    OrbExtractor,
    OrbFeatureDetector,
    OrbParams,
    OrbResult,
    orb_extract_arrays,
)
from .pnp import (  # noqa: F401
    loop_edges_from_pnp,
    p3p_arrays,
    solve_pnp_ransac,
    solve_pnp_ransac_batch,
    solve_pnp_ransac_offsets,
)
from .ba_sparse import SparseBAProblem, bundle_adjust_sparse, covisibility  # noqa: F401
from .covis import CovisibilityGraph, CovisibilityTables, covisibility_device  # noqa: F401
from .bow import (  # noqa: F401
    BowDatabase,
    BowVectors,
    Vocabulary,
    bow_transform,
    bow_vectors,
    detect_loop_candidates,
    read_dbow2_text,
    train_vocabulary,
    write_dbow2_text,
)
from .bow_match import (  # noqa: F401
    FeatureVectors,
    bow_feature_vectors,
    match_index_pairs,
    node_match_arrays,
    node_top2,
    search_by_bow,
    search_by_bow_descriptors,
)
from .proj_match import (  # noqa: F401
    FrameGrids,
    PointSets,
    proj_match_arrays,
    project_points,
    scale_tables,
    search_by_projection,
    search_by_sim3,
)
from .tri_match import (  # noqa: F401
    KeyframeViews,
    create_new_map_points,
    epi_match_arrays,
    epipole_in_second,
    fundamental_from_poses,
    search_for_triangulation,
    triangulate_matches,
)
from .fuse import (  # noqa: F401
    MapObservations,
    apply_fusion,
    fuse_arrays,
    fuse_by_sim3,
    fuse_points,
    refresh_map_points,
)
from .local_map import (  # noqa: F401
    MapTables,
    cull_keyframes,
    cull_map_points,
    frame_points_host,
    keyframe_redundancy,
    keyframe_redundancy_host,
    local_keyframe_votes,
    local_keyframes,
    local_points,
    local_points_host,
    redundant_verdict,
    remove_frames,
    votes_host,
)
from .loop_detect import (  # noqa: F401
    BestTable,
    LoopCandidates,
    LoopConsistency,
    LoopDetector,
    loop_candidates,
    loop_candidates_host,
    loop_candidates_tables,
    relocalization_candidates,
)
from .pose_graph import (  # noqa: F401
    loop_edges_from_two_view,
    optimize_pose_graph,
    pose_graph_hmul,
    pose_graph_linearize,
    pose_graph_pcg,
    read_g2o,
    write_g2o,
)
from .reproj import PoseOnlyProblem, ReprojProblem, build_linearization, poses_to_rt12  # noqa: F401
from .sim3 import (  # noqa: F401
    align_trajectory,
    estimate_sim3,
    estimate_sim3_batch,
    estimate_sim3_offsets,
    fit_sim3,
    fit_sim3_offsets,
    loop_edges_from_sim3,
    sim3_threepoint_arrays,
)
from .sim3_opt import (  # noqa: F401
    compute_sim3,
    optimize_sim3,
    optimize_sim3_batch,
    optimize_sim3_offsets,
    sim3_to_s12,
)
from .camera import (  # noqa: F401
    CameraModel,
    RectifyMap,
    distort_points,
    image_bounds,
    remap_images,
    undistort_points,
)
from .stereo import (  # noqa: F401
    StereoResult,
    stereo_match,
    stereo_match_arrays,
)
from .stereo_opt import (  # noqa: F401
    StereoEdges,
    local_bundle_adjust,
    optimize_poses_stereo,
    stereo_edge_linearization,
    stereo_edges,
)
from .sim3_graph import (  # noqa: F401
    correct_points,
    lift_se3_graph,
    optimize_sim3_graph,
    sim3_edges_from_sim3,
    sim3_graph_hmul,
    sim3_graph_linearize,
    sim3_graph_pcg,
    sims_to_poses,
)
from .two_view import (  # noqa: F401
    estimate_two_view,
    find_essential_arrays,
    find_essential_batch,
    find_essential_offsets,
    fivepoint_arrays,
    mean_reprojection_error,
    recover_pose_arrays,
    recover_pose_batch,
    recover_pose_offsets,
    triangulate_arrays,
    verify_pairs,
)
