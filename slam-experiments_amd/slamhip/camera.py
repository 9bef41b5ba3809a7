"""Lens distortion on the GPU (``slam_cam_*``): what ORB-SLAM does in ``Frame::UndistortKeyPoints`` and
``ComputeImageBounds`` and OpenCV in ``undistortPoints``, ``initUndistortRectifyMap`` and ``remap``.  Every other geometric call
of this package takes a pinhole camera; these bring the keypoints of a real lens (after extraction), or its image (before
extraction), to that camera.

PARITY UNPINNED: cv2 is absent here.  The inverse is Newton's method run for a fixed number of steps, and every point carries
a status (0 converged, 1 not converged, 2 no pinhole image exists, 3 input not finite); for a status other than 0 the outputs
are NaN, never a plausible wrong number.  There is no CPU fallback.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np

from ._args import _Buffers
from ._lib import addr, check
from .device import Context, DeviceBuffer, default_context

MODELS = ("pinhole", "radtan", "equidistant")
N_COEFFS = {"pinhole": 0, "radtan": 5, "equidistant": 4}
RECORD = 16                         # SLAM_CAM_RECORD
MAX_CAMERAS = 8                     # SLAM_CAM_MAX
MAX_ITERATIONS = 100                # SLAM_CAM_ITERATIONS_MAX
MAX_SIDE = 32768                    # SLAM_CAM_SIDE_MAX
DEFAULT_ITERATIONS = 10
MAP_SENTINEL = -2 ** 31
OK, NOT_CONVERGED, NO_IMAGE, NOT_FINITE = 0, 1, 2, 3


class CameraModel:
    """``(fx, fy, cx, cy)`` and a distortion model: ``"pinhole"`` (no coefficients), ``"radtan"`` (OpenCV / Brown-Conrady,
    ``coeffs = (k1, k2, p1, p2[, k3])``) or ``"equidistant"`` (Kannala-Brandt, ``coeffs = (k1, k2, k3, k4)``: cv2.fisheye,
    Kalibr's equidistant, ORB-SLAM3's KannalaBrandt8).  ``record`` is the f64 [16] the library takes."""

    def __init__(self, fx, fy, cx, cy, model: str = "pinhole", coeffs: Sequence[float] = ()):
        if model not in MODELS:
            raise ValueError(f"model must be one of {MODELS}, got {model!r}")
        try:
            K = [float(fx), float(fy), float(cx), float(cy)]
            k = [float(v) for v in coeffs]
        except (TypeError, ValueError) as exc:
            raise ValueError("intrinsics and coefficients must be numbers") from exc
        if not np.isfinite(K + k).all():
            raise ValueError("intrinsics and coefficients must be finite")
        if not (K[0] > 0 and K[1] > 0):
            raise ValueError("fx and fy must be positive")
        want = N_COEFFS[model]
        if model == "radtan" and len(k) == 4:
            k.append(0.0)                                       # k3 is optional, as in OpenCV
        if len(k) != want:
            raise ValueError(f"{model} takes {want} coefficients{' (or 4: k3 = 0)' if model == 'radtan' else ''}, got {len(coeffs)}")
        self.fx, self.fy, self.cx, self.cy = K
        self.model, self.coeffs = model, tuple(k)
        rec = np.zeros(RECORD)
        rec[:4], rec[4] = K, MODELS.index(model)
        rec[5:5 + len(k)] = k
        rec.flags.writeable = False
        self.record = rec

    @property
    def K(self) -> Tuple[float, float, float, float]:
        return (self.fx, self.fy, self.cx, self.cy)

    def pinhole(self) -> "CameraModel":
        """The pinhole camera of the same intrinsics: the camera the undistorted pixels belong to."""
        return CameraModel(*self.K)

    def __repr__(self):
        return f"CameraModel({self.fx}, {self.fy}, {self.cx}, {self.cy}, {self.model!r}, {self.coeffs})"


def _cameras(cameras) -> Tuple[np.ndarray, bool]:
    single = isinstance(cameras, CameraModel)
    cams = [cameras] if single else list(cameras)
    if not cams or not all(isinstance(c, CameraModel) for c in cams):
        raise ValueError("cameras must be a CameraModel or a non-empty sequence of them")
    if len(cams) > MAX_CAMERAS:
        raise ValueError(f"at most {MAX_CAMERAS} cameras per call")
    return np.ascontiguousarray(np.stack([c.record for c in cams])), single


def _points_arg(px, offsets, camera_index, C: int):
    try:
        p = np.asarray(px, np.float64)
    except (TypeError, ValueError) as exc:
        raise ValueError("pixels must be numeric") from exc
    if p.size == 0:
        p = np.zeros((0, 2))
    if p.ndim != 2 or p.shape[1] != 2:
        raise ValueError(f"pixels must have shape [n, 2], got {p.shape}")
    p = np.ascontiguousarray(p)
    n = len(p)
    if n > 1 << 30:
        raise ValueError("at most 2^30 points per call")
    if offsets is None:
        off = np.asarray([0, n], np.int64)
    else:
        off = np.asarray(offsets)
        if off.dtype.kind not in "iu" or off.ndim != 1 or len(off) < 1:
            raise ValueError("offsets must be integers of shape [B + 1]")
        off = np.ascontiguousarray(off, np.int64)
        if off[0] != 0 or off[-1] != n or (np.diff(off) < 0).any():
            raise ValueError(f"offsets must ascend from 0 to {n}")
    B = len(off) - 1
    idx = None
    if camera_index is not None:
        idx = np.asarray(camera_index)
        if idx.dtype.kind not in "iu" or idx.shape != (B,):
            raise ValueError(f"camera_index must be integers of shape [{B}], got {idx.dtype} {idx.shape}")
        if B and (idx.min() < 0 or idx.max() >= C):
            raise ValueError(f"camera_index must lie in [0, {C})")
        idx = np.ascontiguousarray(idx, np.int32)
    return p, off, idx


def _run_points(direction: int, px, cameras, offsets, camera_index, iterations, ctx):
    rec, _ = _cameras(cameras)
    p, off, idx = _points_arg(px, offsets, camera_index, len(rec))
    if isinstance(iterations, bool) or int(iterations) != iterations or not 0 <= iterations <= MAX_ITERATIONS:
        raise ValueError(f"iterations must be an integer in [0, {MAX_ITERATIONS}]")
    n = len(p)
    if n == 0:
        return np.zeros((0, 2)), np.zeros((0, 2)), np.zeros(0, np.uint8)
    ctx = ctx or default_context()
    m = _Buffers(ctx)
    try:
        d_in, d_out, d_norm, d_st = m.up(p), m.new(16 * n), m.new(16 * n), m.new(n)
        cam_idx = addr(idx) if idx is not None and len(idx) else None
        if direction == 0:
            check(ctx.lib.slam_cam_undistort_f64(ctx.handle, len(off) - 1, addr(off), len(rec), addr(rec), cam_idx, int(iterations), d_in.ptr,
                                                 d_out.ptr, d_norm.ptr, d_st.ptr))
        else:
            check(ctx.lib.slam_cam_distort_f64(ctx.handle, len(off) - 1, addr(off), len(rec), addr(rec), cam_idx, d_in.ptr, d_out.ptr, d_norm.ptr,
                                               d_st.ptr))
        return d_out.download(np.float64, (n, 2)), d_norm.download(np.float64, (n, 2)), d_st.download(np.uint8, (n,))
    finally:
        m.free()


def undistort_points(px, cameras, offsets=None, camera_index=None, iterations: int = DEFAULT_ITERATIONS, ctx: Optional[Context] = None):
    """``slam_cam_undistort_f64``: raw pixels f64 [n,2] -> (pinhole pixels f64 [n,2] of the same ``fx..cy``, normalised
    coordinates f64 [n,2], status u8 [n]).  ``cameras``: one ``CameraModel`` or up to 8; set b = ``[offsets[b], offsets[b+1])``
    uses camera ``camera_index[b]`` (None: camera 0; ``offsets`` None: one set).  Outputs are NaN where the status is not 0."""
    return _run_points(0, px, cameras, offsets, camera_index, iterations, ctx)


def distort_points(px, cameras, offsets=None, camera_index=None, ctx: Optional[Context] = None):
    """``slam_cam_distort_f64``: pinhole pixels f64 [n,2] of the same ``fx..cy`` -> (raw pixels f64 [n,2], distorted normalised
    coordinates f64 [n,2], status u8 [n]: 3 and NaN for an input that is not finite, else 0)."""
    return _run_points(1, px, cameras, offsets, camera_index, 0, ctx)


def _size(size, name: str) -> Tuple[int, int]:
    try:
        W, H = size
    except (TypeError, ValueError) as exc:
        raise ValueError(f"{name} must be (W, H)") from exc
    for v in (W, H):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"{name} must be two integers, got {size!r}")
    if not (1 <= W <= MAX_SIDE and 1 <= H <= MAX_SIDE):
        raise ValueError(f"{name} must lie in [1, {MAX_SIDE}], got {size!r}")
    return int(W), int(H)


def image_bounds(camera: CameraModel, size, iterations: int = DEFAULT_ITERATIONS, ctx: Optional[Context] = None):
    """ORB-SLAM's ``ComputeImageBounds``: the raw corners (0,0), (W,0), (0,H), (W,H) of a ``size = (W, H)`` image undistorted,
    ``min_x = min(c00.x, c0H.x)``, ``max_x = max(cW0.x, cWH.x)``, ``min_y = min(c00.y, cW0.y)``, ``max_y = max(c0H.y, cWH.y)``,
    returned as ``(min_x, max_x, min_y, max_y)``: the ``bounds`` of ``search_by_projection`` / ``project_points``.  ValueError
    when a corner has no undistorted image."""
    if not isinstance(camera, CameraModel):
        raise ValueError("camera must be a CameraModel")
    W, H = _size(size, "size")
    corners = np.asarray([[0.0, 0.0], [W, 0.0], [0.0, H], [W, H]], np.float64)
    out, _, st = undistort_points(corners, camera, iterations=iterations, ctx=ctx)
    if st.any():
        raise ValueError(f"the corners of the image have no undistorted image (status {st.tolist()})")
    return (float(min(out[0, 0], out[2, 0])), float(max(out[1, 0], out[3, 0])), float(min(out[0, 1], out[1, 1])),
            float(max(out[2, 1], out[3, 1])))


class RectifyMap:
    """The resident fixed-point map (``slam_cam_rectify_map``) of a ``size_out = (W, H)`` image of the pinhole camera
    ``new_camera`` (None: the pinhole camera of ``camera``'s own intrinsics) turned by ``R`` [3,3] (None: identity) into the
    raw image of ``camera``: int32 [H, W, 2] in 1/32 pixel, ``MAP_SENTINEL`` twice where the ray has no raw pixel."""

    def __init__(self, camera: CameraModel, size_out, new_camera=None, R=None, ctx: Optional[Context] = None):
        if not isinstance(camera, CameraModel):
            raise ValueError("camera must be a CameraModel")
        self.W, self.H = _size(size_out, "size_out")
        if new_camera is None:
            newK = camera.K
        elif isinstance(new_camera, CameraModel):
            if new_camera.model != "pinhole":
                raise ValueError("new_camera must be a pinhole camera")
            newK = new_camera.K
        else:
            newK = tuple(float(v) for v in new_camera)
            if len(newK) != 4 or not np.isfinite(newK).all() or not (newK[0] > 0 and newK[1] > 0):
                raise ValueError("new_camera must be a pinhole CameraModel or finite (fx, fy, cx, cy) with fx, fy > 0")
        self.camera, self.new_K = camera, np.asarray(newK, np.float64)
        self.R = None
        if R is not None:
            r = np.asarray(R, np.float64)
            if r.shape != (3, 3) or not np.isfinite(r).all():
                raise ValueError("R must be a finite [3, 3] matrix")
            self.R = np.ascontiguousarray(r).reshape(9)
        self.ctx = ctx or default_context()
        self.buf: Optional[DeviceBuffer] = self.ctx.malloc(8 * self.W * self.H)
        try:
            check(self.ctx.lib.slam_cam_rectify_map(self.ctx.handle, addr(camera.record), addr(self.R) if self.R is not None else None,
                                                    addr(self.new_K), self.W, self.H, self.buf.ptr))
            self.ctx.sync()
        except BaseException:
            self.free()
            raise

    @property
    def size(self) -> Tuple[int, int]:
        return (self.W, self.H)

    def download(self) -> np.ndarray:
        return self.buf.download(np.int32, (self.H, self.W, 2))

    def free(self) -> None:
        if self.buf is not None:
            self.buf.free()
            self.buf = None


def _check_border(border) -> int:
    if isinstance(border, bool) or not isinstance(border, (int, np.integer)) or not 0 <= border <= 255:
        raise ValueError("border must be an integer in [0, 255]")
    return int(border)


def _check_frames(images) -> np.ndarray:
    a = np.asarray(images)
    if a.dtype != np.uint8:
        raise ValueError(f"images must be uint8, got {a.dtype}")
    if a.ndim == 2:
        a = a[None]
    if a.ndim != 3 or a.shape[1] == 0 or a.shape[2] == 0:
        raise ValueError(f"images must have shape [B, H, W] or [H, W] with H, W > 0, got {a.shape}")
    if a.shape[1] > MAX_SIDE or a.shape[2] > MAX_SIDE:
        raise ValueError(f"image sides must be at most {MAX_SIDE}")
    return np.ascontiguousarray(a)


def remap_device(ctx: Context, src: DeviceBuffer, B: int, Hs: int, Ws: int, rect_map: RectifyMap, dst: DeviceBuffer,
                 mask: Optional[DeviceBuffer] = None, border: int = 0) -> None:
    """``slam_cam_remap_u8`` on resident buffers: ``src`` u8 [B, Hs, Ws] dense, ``dst`` (and ``mask``) u8 [B, H, W] dense of the
    map's size - the layout of an ``OrbExtractor``'s image and mask blocks."""
    W, H = rect_map.size
    if rect_map.buf is None:
        raise ValueError("the map was freed")
    if src.nbytes < B * Hs * Ws or dst.nbytes < B * H * W or (mask is not None and mask.nbytes < B * H * W):
        raise ValueError("a buffer is smaller than its images")
    check(ctx.lib.slam_cam_remap_u8(ctx.handle, src.ptr, B, Hs, Ws, Ws, Hs * Ws, rect_map.buf.ptr, H, W, _check_border(border), dst.ptr, W, H * W,
                                    mask.ptr if mask is not None else None))


def remap_images(images, rect_map: RectifyMap, border: int = 0, with_mask: bool = True):
    """``cv2.remap(image, map, INTER_LINEAR, BORDER_CONSTANT, border)`` of u8 [B,Hs,Ws] (or one [Hs,Ws]) through a
    ``RectifyMap``: (images u8 [B,H,W], mask u8 [B,H,W] or None).  ``mask`` is 255 where every tap that counts lies inside the
    source, else 0 - the detection mask to hand to ORB."""
    a = _check_frames(images)
    border = _check_border(border)
    if not isinstance(rect_map, RectifyMap):
        raise ValueError("rect_map must be a RectifyMap")
    B, Hs, Ws = a.shape
    W, H = rect_map.size
    if B == 0:
        return np.zeros((0, H, W), np.uint8), (np.zeros((0, H, W), np.uint8) if with_mask else None)
    ctx = rect_map.ctx
    m = _Buffers(ctx)
    try:
        d_src, d_dst = m.up(a), m.new(B * H * W)
        d_mask = m.new(B * H * W) if with_mask else None
        remap_device(ctx, d_src, B, Hs, Ws, rect_map, d_dst, d_mask, border)
        out = d_dst.download(np.uint8, (B, H, W))
        return out, (d_mask.download(np.uint8, (B, H, W)) if with_mask else None)
    finally:
        m.free()


def undistort_keypoints(result, camera: CameraModel, iterations: int = DEFAULT_ITERATIONS, ctx: Optional[Context] = None):
    """``Frame::UndistortKeyPoints`` for an ``OrbResult``: (list of f64 [n_b,2] pinhole pixels, list of u8 [n_b] status), all
    images in one call."""
    counts = [len(x) for x in result.xy]
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    px = np.concatenate([np.asarray(x, np.float64).reshape(-1, 2) for x in result.xy]) if counts else np.zeros((0, 2))
    out, _, st = undistort_points(px, camera, off, iterations=iterations, ctx=ctx)
    rng = range(len(counts))
    return [out[off[b]:off[b + 1]].copy() for b in rng], [st[off[b]:off[b + 1]].copy() for b in rng]
