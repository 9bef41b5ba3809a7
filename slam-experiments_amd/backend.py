"""Drop-in for the reference's ``backend.py`` with a GPU-backed ``Backend``.

The reference's ``Backend`` is an empty stub (``backend.py:101-103``) and its
``Map`` container is unrelated to the hot path, so this module

* re-exports the reference's own ``Map`` when a reference ``backend.py`` is
  further down ``sys.path`` (overlay install; nothing is copied), and
* defines ``Backend`` — still zero-argument constructible — with the
  per-observation residual/Jacobian build (``frontend.py:272-291`` arithmetic)
  running on MI355X through ``libslamhip.so``.

No CPU fallback: without the library or a gfx950 GPU the methods raise.
"""
from __future__ import annotations

import ast
import importlib.util
import os
import sys
from typing import Optional

import numpy as np

from slamhip import ba as _ba
from slamhip import ba_sparse as _bas
from slamhip import bow as _bow
from slamhip import covis as _cv
from slamhip import bow_match as _bm
from slamhip import camera as _cam
from slamhip import fuse as _fz
from slamhip import local_map as _lm
from slamhip import loop_detect as _ld
from slamhip import proj_match as _pm
from slamhip import tri_match as _tm
from slamhip import pnp as _pnp
from slamhip import pose_graph as _pg
from slamhip import sim3_graph as _s3g
from slamhip import sim3_opt as _s3o
from slamhip import stereo as _st
from slamhip import stereo_opt as _so
from slamhip import pose_opt as _po
from slamhip import reproj as _r
from slamhip import two_view as _tv
from slamhip.device import Context, default_context

_HERE = os.path.dirname(os.path.abspath(__file__))


# What identifies the reference's backend.py (backend.py:10-12): ``class Map`` whose body sets its two tuning constants.
_REFERENCE_CONSTANTS = ("NUM_ACTIVE_KEYFRAMES", "MIN_DIST_THRESHOLD")


def _assigned_names(body) -> set:
    out = set()
    for node in body:
        targets = node.targets if isinstance(node, ast.Assign) else [node.target] if isinstance(node, ast.AnnAssign) else []
        out.update(t.id for t in targets if isinstance(t, ast.Name))
    return out


def _reference_marks_missing(text: str):
    """What a ``backend.py`` source lacks to be the reference's: a top-level ``class Map`` and the two constants, set
    in the class body as the reference has them (``backend.py:10-12``) or at module level.  Parsed, never executed."""
    try:
        tree = ast.parse(text)
    except SyntaxError as exc:
        return [f"does not parse: {exc.msg}"]
    classes = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "Map"]
    if not classes:
        return ["class Map"]
    have = _assigned_names(tree.body) | _assigned_names(classes[-1].body)
    return [c for c in _REFERENCE_CONSTANTS if c not in have]


def _load_reference_backend():
    """Find the REFERENCE's ``backend.py`` on sys.path and load it; returns (module, report).

    An overlay install puts this directory ahead of the reference's on ``sys.path`` and both files are called
    ``backend.py``.  A candidate is accepted only if its source defines the reference's ``Map`` class with
    ``NUM_ACTIVE_KEYFRAMES`` and ``MIN_DIST_THRESHOLD`` (class attributes, ``backend.py:10-12``) - checked on the
    syntax tree BEFORE anything is executed, so an unrelated ``backend.py`` that happens to be on the path is neither
    imported nor mistaken for it.  The current working directory (the ``''`` entry) is considered only through that
    same test.  ``report`` lists what was looked at, for the error message."""
    seen, report = set(), []
    for entry in sys.path:
        base = os.path.abspath(entry or os.getcwd())
        if base == _HERE or base in seen:
            continue
        seen.add(base)
        cand = os.path.join(base, "backend.py")
        if not os.path.isfile(cand):
            continue
        try:
            with open(cand, encoding="utf-8", errors="replace") as f:
                text = f.read()
        except OSError as exc:
            report.append(f"{cand}: unreadable ({exc})")
            continue
        missing = _reference_marks_missing(text)
        if missing:
            report.append(f"{cand}: not the reference's backend.py (no {', '.join(missing)})")
            continue
        spec = importlib.util.spec_from_file_location("_reference_backend", cand)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        Map = getattr(mod, "Map", None)
        if isinstance(Map, type) and all(hasattr(Map, c) or hasattr(mod, c) for c in _REFERENCE_CONSTANTS):
            return mod, report
        report.append(f"{cand}: its source names Map and the two constants, but executing it did not define them")
    return None, report


def __getattr__(name: str):
    if name == "Map":  # resolved lazily so the module imports without the reference present
        ref, report = _load_reference_backend()
        if ref is None:
            looked = "; ".join(report) if report else "no other backend.py on sys.path"
            raise ImportError("Map lives in the reference's backend.py (class Map + NUM_ACTIVE_KEYFRAMES + "
                              f"MIN_DIST_THRESHOLD), which was not found on sys.path: {looked}")
        globals()["Map"] = ref.Map
        return ref.Map
    raise AttributeError(f"module 'backend' has no attribute {name!r}")


class Backend:
    def __init__(self):
        self._ctx: Optional[Context] = None

    @property
    def ctx(self) -> Context:
        if self._ctx is None:
            self._ctx = default_context()
        return self._ctx

    def build_linearization(self, poses, points, obs_pose_idx, obs_point_idx, meas, fx, fy, cx, cy,
                            with_point: bool = True):
        """Residuals and Jacobians of every observation: (e [O,2], J_pose [O,2,6], J_point [O,2,3])."""
        return _r.build_linearization(poses, points, obs_pose_idx, obs_point_idx, meas, fx, fy, cx, cy,
                                      with_point, self.ctx)

    def estimate_two_view(self, px1, px2, fx, fy, cx, cy, hypotheses: int = _tv.DEFAULT_HYPOTHESES,
                          threshold: float = _tv.DEFAULT_THRESHOLD, seed: int = 0):
        """``pose_estimation_2d2d`` (``utils.py:10-28``: ``cv2.findEssentialMat`` + ``cv2.recoverPose``) on arrays:
        ``px1`` [N,2] the last frame's pixels (``trainIdx``), ``px2`` [N,2] the current frame's (``queryIdx``) ->
        (R [3,3], t [3], RANSAC inlier mask [N]) with ``X2 = R X1 + t``, ``|t| = 1`` - what the reference wraps into an
        ``SE3`` as the relative motion (``frontend.py:119-120``)."""
        return _tv.estimate_two_view(px1, px2, (fx, fy, cx, cy), hypotheses, threshold, seed, ctx=self._ctx)

    def verify_pairs(self, pairs, fx, fy, cx, cy, hypotheses: int = _tv.DEFAULT_HYPOTHESES,
                     threshold: float = _tv.DEFAULT_THRESHOLD, seed: int = 0):
        """Geometric verification of many candidate frame pairs in one call (loop-closure or relocalisation candidates
        from ``KeyframeDatabase``): ``pairs`` = list of ``(px1 [N_b,2], px2 [N_b,2])`` -> (poses [B,4,4] mapping frame 1 to
        frame 2, inlier counts [B], list of inlier masks).  A pair of fewer than five matches (``frontend.py:116``) comes
        back with the identity and a count of 0."""
        R, t, masks, counts = _tv.verify_pairs(pairs, (fx, fy, cx, cy), hypotheses, threshold, seed, ctx=self._ctx)
        poses = np.tile(np.eye(4), (len(R), 1, 1))
        poses[:, :3, :3] = R
        poses[:, :3, 3] = t
        return poses, counts, masks

    def relocalize(self, candidates, fx, fy, cx, cy, hypotheses: int = _pnp.DEFAULT_HYPOTHESES,
                   threshold: float = _pnp.DEFAULT_THRESHOLD, seed: int = 0, refine: bool = True):
        """Absolute pose of the current frame against many candidate keyframes in one call (what
        ``Frontend._reinitialize_from_keyframe``, ``frontend.py:223-229``, lacks and drops the map for): ``candidates`` =
        list of ``(map points [N_b,3], pixels [N_b,2])``, the candidate's map points matched in the current frame ->
        (poses [B,4,4] world -> camera, inlier counts [B], list of inlier masks).  P3P RANSAC, then (``refine``) the pose-only
        optimisation of ``correct_frame_pose`` on the inliers.  A candidate of fewer than three correspondences, or
        without a model, comes back with the identity and a count of 0."""
        T, masks, counts, _, _ = _pnp.solve_pnp_ransac_batch(candidates, (fx, fy, cx, cy), hypotheses, threshold, seed, refine, ctx=self._ctx)
        poses = np.tile(np.eye(4), (len(T), 1, 1))
        poses[:, :3, :] = T
        return poses, counts, masks

    def detect_loop_candidates(self, db, vector, connected=(), min_score: float = 0.0):
        """The first stage of ORB-SLAM's ``DetectLoopCandidates`` on a ``slamhip.BowDatabase`` (the reference detects no
        loops): dense scores and shared-word counts of ``vector`` against every entry come from the device; the ``connected``
        ids are dropped, and the entries with more than 0.8 of the largest shared-word count and a score of at least
        ``min_score`` are returned as (ids, scores) by (score descending, id ascending) - the candidates ``relocalize`` and
        ``estimate_sim3_batch`` take."""
        return _bow.detect_loop_candidates(db, vector, connected, min_score)

    def detect_loop(self, db, vectors, graph_or_best_table, connected=None, own_ids=None, limit=None, min_score=None, nb: int = 10):
        """ORB-SLAM's whole ``DetectLoopCandidates`` for Q BoW ``vectors`` at once (the reference detects no loops): the dense
        query and the covisibility-group stage stay on the device - per query the entries that are not ``connected`` (nor
        ``own_ids``), lie below ``limit``, share more than 0.8 of the largest shared-word count and score at least
        ``min_score`` (None: the lowest score against the connected keyframes) are summed with their ``nb`` best covisibles,
        the groups within 0.75 of the best are kept and each gives its best-scoring member ->
        ``slamhip.LoopCandidates`` (``offsets``, ``ids`` ascending, ``scores`` as ``s_int``).  Feed the ids of consecutive
        keyframes to a ``slamhip.LoopConsistency``, or let a ``slamhip.LoopDetector`` do both."""
        return _ld.loop_candidates(db, vectors, graph_or_best_table, connected, own_ids, limit, min_score, nb)

    def detect_relocalization_candidates(self, db, vectors, best_table, nb: int = 10):
        """``DetectRelocalizationCandidates`` for Q lost frames at once: as ``detect_loop`` without excluded keyframes and
        without a threshold on the score -> ``slamhip.LoopCandidates``, the keyframes ``relocalize`` tries."""
        return _ld.relocalization_candidates(db, vectors, best_table, nb)

    def compute_sim3(self, cands, K, min_inliers: int = _s3o.DEFAULT_MIN_INLIERS, **kw):
        """The estimation half of ORB-SLAM's ``LoopClosing::ComputeSim3`` (the reference closes no loops): ``cands`` = list of
        ``(X1 [N_b,3], X2 [N_b,3], px1 [N_b,2], px2 [N_b,2][, sigma2 [N_b,2]])``, the matched map points of a loop candidate
        in their own camera frames and their measured keypoints -> ``estimate_sim3_batch`` (RANSAC + refit), then
        ``optimize_sim3_batch`` (the reprojection refinement, ``Optimizer::OptimizeSim3``) on the RANSAC inliers.  Returns
        (models = (s, R, t) with ``X2 = s R X1 + t``, what ``sim3_edges_from_sim3`` takes; masks over each candidate's own
        indexing; counts [B]; accepted bool [B] = count >= ``min_inliers``, ORB-SLAM's 20).  ``slamhip.sim3_to_s12`` turns a
        model into what ``search_by_sim3`` and ``fuse_by_sim3`` take."""
        models, masks, counts, accepted, _ = _s3o.compute_sim3(cands, K, min_inliers, ctx=self._ctx, **kw)
        return models, masks, counts, accepted

    def undistort_points(self, px, camera, offsets=None, camera_index=None, iterations: int = _cam.DEFAULT_ITERATIONS):
        """``Frame::UndistortKeyPoints`` (the reference works on raw ``keypoint.pt`` and has no counterpart): raw pixels [n,2]
        under a ``slamhip.CameraModel`` (or up to 8, selected per set) -> (pinhole pixels [n,2], status u8 [n]); NaN where
        the status is not 0 (1 not converged, 2 beyond the fold of the model, 3 input not finite)."""
        out, _, status = _cam.undistort_points(px, camera, offsets, camera_index, iterations, ctx=self._ctx)
        return out, status

    def image_bounds(self, camera, size, iterations: int = _cam.DEFAULT_ITERATIONS):
        """``Frame::ComputeImageBounds``: (min_x, max_x, min_y, max_y) of the undistorted corners of a ``size = (W, H)`` image,
        the ``bounds`` of ``match_by_projection``'s searches."""
        return _cam.image_bounds(camera, size, iterations, ctx=self._ctx)

    def stereo_frame(self, left, right=None, pairs=None, *, bf, fx=None, **kw):
        """ORB-SLAM's ``Frame::ComputeStereoMatches`` (the reference opens one camera and has no counterpart): ``left`` and
        ``right`` are ``slamhip.OrbExtractor``s of the rectified images after ``run()`` - or one extractor and ``pairs`` =
        (left image, right image) inside it - and ``bf`` the focal length times the baseline.  Returns a
        ``slamhip.StereoResult``: per pair ``u_right``, ``depth`` and a status for every left keypoint; its ``points`` and
        ``point_set`` turn the matched rows into camera-frame or world points."""
        return _st.stereo_match(left, right, pairs, bf=bf, fx=fx, **kw)

    def track_stereo_pose(self, poses, points_list, edges_list, fx, fy, cx, cy, bf, rounds: int = 4, iterations: int = 10,
                          gates=(_so.CHI2_MONO, _so.CHI2_STEREO), deltas=(_so.DELTA_MONO, _so.DELTA_STEREO)):
        """ORB-SLAM's ``Optimizer::PoseOptimization`` with monocular and stereo edges mixed and every edge weighted by its
        pyramid level, for several frames in one launch: ``edges_list[b]`` is a ``slamhip.StereoEdges``
        (``slamhip.stereo_edges`` builds one from a ``stereo_frame`` result), ``points_list[b]`` the map points of its rows.
        Returns a list of ``PoseOptResult`` (``slamhip.optimize_poses_stereo``)."""
        return _so.optimize_poses_stereo(poses, points_list, edges_list, (fx, fy, cx, cy), bf, rounds, iterations, gates, deltas, ctx=self.ctx)

    def local_bundle_adjust(self, poses, points, obs_pose_idx, obs_point_idx, stereo, fx, fy, cx, cy, fixed_poses=(0,), first: int = 5,
                            second: int = 10, gates=(_so.CHI2_MONO, _so.CHI2_STEREO), deltas=(_so.DELTA_MONO, _so.DELTA_STEREO)):
        """ORB-SLAM's ``Optimizer::LocalBundleAdjustment`` over a window: the sparse adjustment with stereo / level-weighted edges
        (``stereo``: a ``slamhip.StereoEdges`` over the observations) and the two-stage outlier schedule.  Returns
        (``slamhip.ba.BAResult``, outlier observation indices, stats dict) (``slamhip.local_bundle_adjust``)."""
        return _so.local_bundle_adjust(poses, points, obs_pose_idx, obs_point_idx, stereo, (fx, fy, cx, cy), fixed_poses, first, second,
                                       gates, deltas, ctx=self.ctx)

    def match_by_bow(self, keyframes, frame, candidates, frame_index: int = 0, keyframe_bins=None, frame_bins=None,
                     th_low: int = _bm.TH_LOW, ratio: float = _bm.RATIO):
        """ORB-SLAM's ``ORBmatcher::SearchByBoW`` of one frame against its candidate keyframes, the step after
        ``detect_loop_candidates``: ``keyframes`` and ``frame`` are ``slamhip.FeatureVectors`` (``bow_feature_vectors``),
        ``candidates`` the keyframe ids, ``frame_index`` the image of ``frame``; the bins (``OrbResult.bin`` of every row of
        the two sets) switch the rotation check on.  Returns per candidate ``(i1, i2)``: int32 arrays of the matched keyframe
        rows (ascending) and frame rows, so that ``(map_points_of_keyframe[i1], frame_pixels[i2])`` is one entry of
        ``relocalize``'s ``candidates`` and ``(points_of_keyframe[i1], points_of_frame[i2])`` one pair of
        ``estimate_sim3_batch``."""
        cand = np.asarray(list(candidates), np.int64).reshape(-1)
        pairs = np.stack([cand, np.full(len(cand), int(frame_index), np.int64)], axis=1) if len(cand) else np.zeros((0, 2), np.int64)
        matches, _ = _bm.search_by_bow(keyframes, frame, pairs, keyframe_bins, frame_bins, th_low, ratio, ctx=self._ctx)
        return _bm.match_index_pairs(matches)

    def match_by_projection(self, points, frames, candidates, poses, fx, fy, cx, cy, frame_index: int = 0, th: float = 15.0,
                            th_high: int = _pm.TH_HIGH, ratio: float = _pm.RATIO, scale=None, bounds=None, centres=None):
        """ORB-SLAM's ``ORBmatcher::SearchByProjection`` of the map points of candidate keyframes into one frame under a
        first pose each - the step after ``relocalize``'s PnP or a motion-model prediction: ``points`` is a
        ``slamhip.PointSets`` (one set per keyframe), ``frames`` a ``slamhip.FrameGrids``, ``candidates`` the point-set ids,
        ``poses`` [C,3,4] or [C,4,4] the world -> camera estimate of the frame for each candidate, ``frame_index`` the image of
        ``frames``.  Returns per candidate ``(i1, i2)``: int32 arrays of the matched points (ascending) and frame rows, as
        ``match_by_bow`` does: ``(xyz_of_set[i1], frame_pixels[i2])`` is one entry of ``relocalize``'s ``candidates`` or the
        input of ``correct_frame_pose`` / ``optimize_pose``, ``(xyz_of_set[i1], points_of_frame[i2])`` one pair of
        ``estimate_sim3_batch``."""
        cand = np.asarray(list(candidates), np.int64).reshape(-1)
        pairs = np.stack([cand, np.full(len(cand), int(frame_index), np.int64)], axis=1) if len(cand) else np.zeros((0, 2), np.int64)
        matches, _ = _pm.search_by_projection(points, frames, pairs, poses, centres, (fx, fy, cx, cy), bounds, scale, th, th_high, ratio,
                                              ctx=self._ctx)
        return _pm.match_index_pairs(matches)

    def create_new_map_points(self, keyframes, new: int, neighbours, poses, fx, fy, cx, cy, views=None, bins=None, scale=None,
                              th_low: int = _tm.TH_LOW):
        """ORB-SLAM's ``LocalMapping::CreateNewMapPoints`` for keyframe ``new`` against its covisible ``neighbours`` (the caller
        passes the neighbours worth searching: the baseline-to-depth gate is not applied): ``keyframes`` is a
        ``slamhip.FeatureVectors`` of all of them, ``views`` the ``slamhip.KeyframeViews`` of the same rows (pixels, levels and
        the rows that already have a map point), ``poses`` [K,3,4] or [K,4,4] world -> camera per keyframe, ``bins`` the
        orientation bins of every row (the rotation check) or None.  ``SearchForTriangulation`` and the per-match checks run as
        one chain of launches.  Returns per neighbour ``(i1, i2, X)``: the rows of ``new`` (ascending) and of the neighbour of
        every created point and its position f64 [.,3]."""
        if views is None:
            raise ValueError("create_new_map_points needs the KeyframeViews of the keyframes (views=)")
        nb = np.asarray(list(neighbours), np.int64).reshape(-1)
        pairs = np.stack([np.full(len(nb), int(new), np.int64), nb], axis=1) if len(nb) else np.zeros((0, 2), np.int64)
        T = np.asarray(poses, np.float64)
        pts, _, _ = _tm.create_new_map_points(keyframes, keyframes, pairs, views, views, T[np.full(len(nb), int(new), np.int64)], T[nb],
                                              (fx, fy, cx, cy), scale, bins, bins, th_low, ctx=self._ctx)
        out = []
        for d in pts:
            i1 = np.flatnonzero(d["status"] == 0).astype(np.int32)
            out.append((i1, d["matches12"][i1], d["X"][i1]))
        return out

    def search_in_neighbors(self, points, ids, frames, frame_points, obs, xyz, new: int, neighbours, poses, fx, fy, cx, cy, scale=None,
                            th: float = _fz.TH, th_low: int = _fz.TH_LOW, ref=None):
        """ORB-SLAM's ``LocalMapping::SearchInNeighbors`` for keyframe ``new`` and its ``neighbours``: ``points`` is a
        ``slamhip.PointSets`` with one set per keyframe (the map points it observes; ``ids`` their map-point ids), ``frames``
        the ``slamhip.FrameGrids`` of the same keyframes built without taken marks, ``frame_points`` the map point of every
        frame row (-1: none), ``obs`` the ``slamhip.MapObservations`` of the map, ``xyz`` f64 [M,3] its positions, ``poses``
        [K,3,4] or [K,4,4] world -> camera per keyframe.  Both directions - the points of ``new`` into every neighbour and the
        points of every neighbour into ``new`` - run as one ``fuse_points`` call; ``apply_fusion`` merges the links; the
        survivors whose observations changed get a new descriptor, normal and distance range (``refresh_map_points``).
        Returns a dict: ``observations`` (the new table), ``alias`` int32 [M], ``updates`` int32 [K,3] = (frame, row, id),
        ``touched`` int32 (the refreshed map points), ``points`` (a ``PointSets`` of them: one set, in ``touched`` order, None
        when nothing changed), ``refresh`` (the arrays ``refresh_map_points`` returned) and ``counts`` int32 [P,3]."""
        nb = np.asarray(list(neighbours), np.int64).reshape(-1)
        k = np.full(len(nb), int(new), np.int64)
        pairs = np.concatenate([np.stack([k, nb], 1), np.stack([nb, k], 1)]) if len(nb) else np.zeros((0, 2), np.int64)
        T = np.asarray(poses, np.float64)
        res, counts = _fz.fuse_points(points, ids, frames, frame_points, obs, pairs, T[pairs[:, 1]], None, (fx, fy, cx, cy), None, scale, th,
                                      th_low, ctx=self._ctx)
        table, alias, updates = _fz.apply_fusion(obs, res)
        touched = np.flatnonzero((table.nobs != obs.nobs) & (alias == np.arange(len(obs)))).astype(np.int32)
        out = dict(observations=table, alias=alias, updates=updates, touched=touched, points=None, refresh=None, counts=counts)
        if len(touched):
            X = np.asarray(xyz, np.float64).reshape(-1, 3)
            r = _fz.refresh_map_points(X, table, frames, _pm.camera_centres(T[:, :3, :]), ref, scale, touched, ctx=self._ctx)
            out["refresh"] = r
            out["points"] = _pm.PointSets(X[touched], r["descriptors"], dmin2=r["dmin2"], dmax2=r["dmax2"], normal=r["normal"], ctx=self._ctx)
        return out

    def triangulate(self, pose1, pose2, px1, px2, fx, fy, cx, cy, reference_projection: bool = False):
        """``triangulation`` (``utils.py:32-55``) on arrays: the poses (4x4 or 3x4 Tcw) of the source and the query frame
        and their matched pixels -> (points [N,3], px1_normalised [N,2]), the reference's return pair.  The pixels are
        normalised (``Camera.pixel_to_camera``) and triangulated against the projections ``pose[:3]``.  The reference
        hands ``cv2.triangulatePoints`` the projections ``K @ pose[:3]`` (``primitives.py:31-32``) together with
        NORMALISED points, i.e. applies the intrinsics twice; ``reference_projection=True`` reproduces that."""
        K = np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])
        P = [np.asarray(p, np.float64).reshape(-1, 4)[:3, :4] for p in (pose1, pose2)]
        if reference_projection:
            P = [K @ p for p in P]
        px1, px2 = _tv._points(px1, "px1"), _tv._points(px2, "px2")
        x1 = np.stack([(px1[:, 0] - cx) / fx, (px1[:, 1] - cy) / fy], 1)
        x2 = np.stack([(px2[:, 0] - cx) / fx, (px2[:, 1] - cy) / fy], 1)
        X, _ = _tv.triangulate_arrays(P[0], P[1], x1, x2, ctx=self._ctx)
        return X, x1

    def mean_reprojection_error(self, points, px, pose, fx, fy, cx, cy) -> float:
        """``Frontend._get_reprojection_error`` (``frontend.py:216-222``) from the residual kernel."""
        return _tv.mean_reprojection_error(points, px, pose, (fx, fy, cx, cy), ctx=self._ctx)

    def optimize_pose(self, pose, points, meas, fx, fy, cx, cy, rounds: int = 4, iterations: int = 10,
                      on_device: bool = True):
        """Pose-only refinement of one frame against its map points: the job of
        ``Frontend._correct_current_pose`` (``frontend.py:298-393``).  With ``on_device`` (default) the whole
        four-round LM loop is one kernel launch; otherwise the host drives it and the GPU evaluates every
        residual, Jacobian and 6x6 system.  Returns ``slamhip.pose_opt.PoseOptResult``."""
        fn = _po.optimize_pose_only_device if on_device else _po.optimize_pose_only
        return fn(pose, points, meas, (fx, fy, cx, cy), rounds, iterations, ctx=self.ctx)

    def optimize_poses(self, poses, points_list, meas_list, fx, fy, cx, cy, rounds: int = 4, iterations: int = 10):
        """``optimize_pose`` for several independent frames in ONE kernel launch (one workgroup per frame): e.g. every
        keyframe of the window against the fixed map, or relocalisation candidates.  Returns a list of
        ``PoseOptResult``, identical to calling ``optimize_pose`` on each frame."""
        return _po.optimize_poses_batch(poses, points_list, meas_list, (fx, fy, cx, cy), rounds, iterations, ctx=self.ctx)

    def optimize(self, poses, points, obs_pose_idx, obs_point_idx, meas, fx, fy, cx, cy, iterations: int = 10,
                 fixed_poses=(0,), huber_delta: float = 0.0, on_device: bool = True):
        """Bundle adjustment over a window of keyframes and their landmarks (``optimizer.optimize(10)`` in
        spirit, ``frontend.py:362``; the reference's ``Backend`` has no body, ``backend.py:101-103``).

        With ``on_device`` (default) a window of at most 16 moving poses and 131 072 observations (the reference keeps
        7 keyframes, ``backend.py:11``) is optimised in ONE kernel launch (``slam_ba_optimize_f64``: the whole LM loop,
        dense solve included, on the device); larger windows run the linearisation, the elimination of the landmarks,
        the blocks of the reduced camera system and the back-substitution on the GPU (``slam_ba_reduce_f64`` /
        ``slam_ba_backsub_f64``) and solve the 6K x 6K system on the host - also what a one-launch attempt falls back to when it
        reports a busy device (``slamhip.SlamHipBusy``).  With ``on_device=False`` only residuals
        and Jacobians come from the GPU and numpy does the rest.  Returns ``slamhip.ba.BAResult``."""
        fn = _ba.bundle_adjust
        if on_device:
            n_free = len(poses) - len(set(fixed_poses))
            one_launch = n_free <= _ba.ONE_LAUNCH_MAX_FREE and len(obs_pose_idx) <= _ba.ONE_LAUNCH_MAX_OBS and len(poses) <= 64
            # the one-launch form needs all its workgroups resident at once; when the device is busy with the tracking
            # thread's work (slam.py:27-35) it gives up in bounded time (SlamHipBusy) and bundle_adjust_auto runs the
            # per-phase kernels instead, once: the adjustment is slower then, it does not fail
            fn = _ba.bundle_adjust_auto if one_launch else _ba.bundle_adjust_device
        return fn(poses, points, obs_pose_idx, obs_point_idx, meas, (fx, fy, cx, cy), iterations, fixed_poses,
                  huber_delta, ctx=self.ctx)

    def global_bundle_adjust(self, poses, points, obs_pose_idx, obs_point_idx, meas, fx, fy, cx, cy, iterations: int = 10,
                             fixed_poses=(0,), huber_delta: float = 0.0, pcg_tol: float = _bas.DEFAULT_PCG_TOL,
                             pcg_max_iter: int = _bas.DEFAULT_PCG_MAX_ITER, covisibility: str = "host"):
        """Bundle adjustment over a whole map (ORB-SLAM's step after a closed loop; the reference's ``Backend`` has no
        body, ``backend.py:101-103``): the arguments of ``optimize``, for thousands of keyframes.  The reduced camera
        system is kept as 6x6 blocks over the covisibility graph and solved by the pose-graph PCG on the device
        (``slamhip.bundle_adjust_sparse``); ``optimize`` and its routing are not involved.  ``covisibility="device"`` builds
        the covisibility tables on the device too (``slamhip.covis``): the same tables and the same result, bit for bit.
        Returns (``slamhip.ba.BAResult``, stats dict)."""
        return _bas.bundle_adjust_sparse(poses, points, obs_pose_idx, obs_point_idx, meas, (fx, fy, cx, cy), iterations, fixed_poses,
                                         huber_delta, pcg_tol, pcg_max_iter, ctx=self.ctx, covisibility=covisibility)

    def covisibility_graph(self, obs_pose_idx, obs_point_idx, K: int, fixed=None):
        """ORB-SLAM's covisibility graph over ``K`` keyframes (``KeyFrame::UpdateConnections`` for the whole map; the reference
        keeps none): an edge between two keyframes that observe a common point, weighted by the number of such points, built on
        the device (``slamhip.covisibility_device``).  Returns ``slamhip.CovisibilityGraph``: ``best(k, n)`` are the neighbours
        ``create_new_map_points`` / ``search_in_neighbors`` search, ``connected(k)`` the ids ``detect_loop_candidates`` skips,
        ``essential_edges()`` the edges of ``optimize_essential_graph``.  ``fixed`` (a mask [K]) leaves poses out."""
        tab = _cv.covisibility_device(obs_pose_idx, obs_point_idx, K, fixed, ctx=self.ctx)
        try:
            return tab.graph()
        finally:
            tab.free()

    def essential_graph_edges(self, obs_pose_idx, obs_point_idx, K: int, min_weight: int = 100, loop_edges=()):
        """The edges of ORB-SLAM's essential graph, int32 [.,2] with k1 < k2, ascending: the spanning tree of the covisibility
        graph, its edges of at least ``min_weight`` common points and ``loop_edges``
        (``covisibility_graph(...).essential_edges``)."""
        return self.covisibility_graph(obs_pose_idx, obs_point_idx, K).essential_edges(min_weight, loop_edges)

    def local_map(self, tables, graph, query_points, limit: int = 80, best: int = 10):
        """ORB-SLAM's ``Tracking::UpdateLocalMap`` for one frame: ``tables`` a ``slamhip.MapTables``, ``graph`` the
        ``slamhip.CovisibilityGraph`` of the same keyframes, ``query_points`` the map points the frame tracks (-1: none).  The
        vote and the local points run on the device (``slamhip.local_keyframe_votes`` / ``local_points``), the expansion over
        the graph on the host (``slamhip.local_keyframes``).  Returns (local keyframes int32, reference keyframe or -1, local
        map points int32, ascending, without the tracked ones): the point set ``match_by_projection`` searches next."""
        votes = _lm.local_keyframe_votes(tables, [np.asarray(query_points).reshape(-1)])
        keyframes, reference = _lm.local_keyframes(votes, graph, limit, best, frame_removed=tables.frame_removed)
        points = _lm.local_points(tables, [keyframes], [np.asarray(query_points).reshape(-1)])[0]
        return keyframes, reference, points

    def cull_keyframes(self, tables, graph, new_keyframe: int, ratio=(9, 10), th_obs: int = 3, protect=(0,)):
        """ORB-SLAM's ``LocalMapping::KeyFrameCulling`` after ``new_keyframe`` was inserted: the candidates are its connected
        keyframes (``graph.connected``), judged one after the other against the map as the earlier removals left it
        (``slamhip.cull_keyframes``).  Returns the removed keyframes int32; ``tables.frame_removed`` holds them on both sides."""
        return _lm.cull_keyframes(tables, graph.connected(new_keyframe), ratio, th_obs, True, protect)

    def optimize_pose_graph(self, poses, edges, meas, info, fixed=(0,), iterations: int = _pg.DEFAULT_ITERATIONS,
                            huber_delta: float = 0.0, pcg_tol: float = _pg.DEFAULT_PCG_TOL,
                            pcg_max_iter: int = _pg.DEFAULT_PCG_MAX_ITER):
        """Pose-graph optimisation over keyframe poses (``pose_graph_sphere_example.py:24-57``: ``VertexSE3`` /
        ``EdgeSE3``, vertex 0 fixed, 15 LM iterations): ``poses`` [V,4,4] / [V,3,4] Tcw, ``edges`` [E,2], ``meas`` the
        measured ``T_j T_i^-1`` per edge (``Frontend._relative_motion``, ``verify_pairs``), ``info`` [E,6,6] in
        ``[w, v]`` order, ``fixed`` the vertex indices (or a bool mask of length V) that hold the gauge.
        Returns (poses in the input's format, stats dict) from ``slamhip.optimize_pose_graph``."""
        V = len(poses)
        fx = np.asarray(fixed)
        if fx.dtype == bool:
            mask = fx.astype(np.uint8)
        else:
            mask = np.zeros(V, np.uint8)
            mask[np.asarray(fixed, np.int64).reshape(-1)] = 1
        return _pg.optimize_pose_graph(poses, edges, meas, info, mask, iterations, huber_delta, pcg_tol, pcg_max_iter, ctx=self.ctx)

    def optimize_essential_graph(self, sims, edges, meas, info, fixed=(0,), iterations: int = _pg.DEFAULT_ITERATIONS,
                                 huber_delta: float = 0.0, pcg_tol: float = _pg.DEFAULT_PCG_TOL,
                                 pcg_max_iter: int = _pg.DEFAULT_PCG_MAX_ITER, fix_scale: bool = False):
        """7-DoF pose-graph optimisation over keyframe similarities (ORB-SLAM's ``OptimizeEssentialGraph``): ``sims``
        [V,13] (``[R|t]`` then ``s``) or the tuple ``(s, R, t)``, ``edges`` [E,2], ``meas`` the measured ``S_j S_i^-1`` per
        edge (``estimate_sim3_batch`` models, ``lift_se3_graph`` for odometry), ``info`` [E,7,7] in ``[w, v, sigma]`` order,
        ``fixed`` the vertex indices (or a bool mask of length V) that hold the gauge.
        Returns (sims in the input's form, stats dict) from ``slamhip.optimize_sim3_graph``."""
        V = len(sims[0]) if _s3g.is_srt(sims) else len(sims)
        fx = np.asarray(fixed)
        if fx.dtype == bool:
            mask = fx.astype(np.uint8)
        else:
            mask = np.zeros(V, np.uint8)
            mask[np.asarray(fixed, np.int64).reshape(-1)] = 1
        return _s3g.optimize_sim3_graph(sims, edges, meas, info, mask, iterations, huber_delta, pcg_tol, pcg_max_iter, fix_scale, ctx=self.ctx)

    def optimize_map(self, map_, fx, fy, cx, cy, iterations: int = 10, huber_delta: float = 5.991 ** 0.5,
                     n_fixed: int = 1, min_observations: int = 2, on_device: bool = True):
        """``optimize`` over the reference's own containers: the active keyframes of a ``Map``
        (``backend.py:10-53``, at most ``NUM_ACTIVE_KEYFRAMES`` = 7) and the landmarks they observe.

        Reads ``map_._active_keyframes`` / ``map_._active_landmarks`` directly — the public getters return deep
        copies (``backend.py:43-53``), which cannot be written back.  An observation is a ``Feature`` in a
        landmark's ``observations`` (``primitives.py:133-147``) whose ``frame`` is an active keyframe; its pixel is
        ``Feature.position`` (int-truncated, ``primitives.py:110-112``).  The ``n_fixed`` oldest keyframes (by
        ``keyframe_id``) hold the gauge.  Landmarks seen fewer than ``min_observations`` times in the window are
        left alone.  Results go back through ``Frame.set_pose`` (as ``type(pose).from_matrix(T)`` when the pose
        class has it, e.g. ``jaxlie.SE3``, else the 4x4 matrix) and ``MapPoint.set_position``.
        Returns ``slamhip.ba.BAResult`` or None if the window holds nothing to optimise."""
        kfs = sorted(map_._active_keyframes.values(), key=lambda f: f.keyframe_id)
        if len(kfs) < 2:
            return None
        kf_index = {id(f): k for k, f in enumerate(kfs)}
        points, landmarks, op, ol, meas = [], [], [], [], []
        for mp in map_._active_landmarks.values():
            obs = [(kf_index[id(ft.frame)], ft) for ft in list(mp.get_observations()) if id(ft.frame) in kf_index]
            if len(obs) < min_observations or len({k for k, _ in obs}) != len(obs):
                continue                                   # too few views, or two features of one frame on one landmark
            l = len(landmarks)
            landmarks.append(mp)
            points.append(np.asarray(mp.position, np.float64))
            for k, ft in sorted(obs, key=lambda kv: kv[0]):
                op.append(k)
                ol.append(l)
                meas.append(np.asarray(ft.position, np.float64))
        if not landmarks:
            return None

        def as_matrix(pose):
            return np.asarray(pose.as_matrix() if hasattr(pose, "as_matrix") else pose, np.float64)

        T = np.stack([as_matrix(f.pose) for f in kfs])
        res = self.optimize(T, np.stack(points), np.asarray(op, np.int32), np.asarray(ol, np.int32), np.stack(meas),
                            fx, fy, cx, cy, iterations=iterations, fixed_poses=tuple(range(min(n_fixed, len(kfs)))),
                            huber_delta=huber_delta, on_device=on_device)
        for k, f in enumerate(kfs[n_fixed:], start=n_fixed):
            make = getattr(type(f.pose), "from_matrix", None)
            f.set_pose(make(res.poses[k]) if make is not None else res.poses[k])
        for l, mp in enumerate(landmarks):
            mp.set_position(res.points[l])
        return res

    def correct_frame_pose(self, frame, fx, fy, cx, cy, rounds: int = 4, iterations: int = 10) -> int:
        """``Frontend._correct_current_pose`` (``frontend.py:298-393``) on the reference's own ``Frame``: one
        edge per feature that has a map point (``:318-320``), landmark position and int pixel as the edge data
        (``:340,348``), four rounds of ten LM iterations with the chi2 gate and the Huber kernel of
        ``optimize_pose``; then the frame takes the refined pose (``:384``), outlier features lose their map
        point and their flag is cleared (``:388-391``).  Returns the inlier count like the reference (``:393``)."""
        features = [ft for ft in frame.features if ft.map_point]
        if not features:
            return 0
        points = np.stack([np.asarray(ft.map_point.position, np.float64) for ft in features])
        pixels = np.stack([np.asarray(ft.position, np.float64) for ft in features])
        pose = frame.pose
        T0 = np.asarray(pose.as_matrix() if hasattr(pose, "as_matrix") else pose, np.float64)
        res = self.optimize_pose(T0, points, pixels, fx, fy, cx, cy, rounds=rounds, iterations=iterations)
        make = getattr(type(pose), "from_matrix", None)
        frame.set_pose(make(res.pose) if make is not None else res.pose)
        for ft, inlier in zip(features, res.inliers):
            if not inlier:
                ft.map_point = None
            ft.is_outlier = False
        return res.n_inliers
