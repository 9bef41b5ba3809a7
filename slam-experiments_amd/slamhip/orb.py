"""ORB feature extraction on the GPU (``slam_orb_*``): what the reference gets from ``cv2.ORB`` behind ``OrbFeatureDetector``
(``feature_detectors.py:18-26``), called on every frame by ``Frontend._detect_features`` (``frontend.py:245``).

PARITY UNPINNED: cv2 is absent here and OpenCV's learned sampling pattern is not shipped, so this is ORB's algorithm (oFAST,
Harris ranking, intensity-centroid orientation, steered BRIEF with a discretised angle) under the integer-exact specification
of DESIGN.md 4d, not ``cv2.ORB``'s output.  The sampling pattern is an argument.  There is no CPU fallback.

``distribution="quadtree"`` replaces the per-level Harris selection by ORB-SLAM's two remedies against features
that crowd on one object: cells without a corner at ``fast_threshold`` keep their corners down to ``fast_threshold_min``, and
the quota is spread over the level by a quadtree.  It runs through ``slam_orb_extract_dist_u8`` on device-resident buffers.
"""
from __future__ import annotations

import ctypes
from typing import List, Optional, Sequence, Tuple

import numpy as np

from ._lib import addr, check, load
from .device import Context, DeviceBuffer, default_context

BORDER = 16                 # no keypoint closer than this to a level's edge
PATTERN_RADIUS = 15         # every pattern point has Euclidean norm <= 15
N_BINS = 32                 # orientation bins of 11.25 degrees
MAX_LEVELS = 16
MAX_SIDE = 8192
MAX_FEATURES = 65536
DISTRIBUTIONS = ("harris", "quadtree")

# The default 256 comparison pairs (ax, ay, bx, by), int8: drawn once from a seeded isotropic Gaussian (sigma 31/5, rounded,
# points beyond radius 15 and pairs closer than 2 pixels redrawn) and committed as numbers, 64 pairs per line.
_DEFAULT_PATTERN_HEX = (
    "fe0204fa07fa0b07fc0403f504fcfefcfd0001f6fef8f8fe0504fcfcfb010600040209f4f3ff04fd03f9f8fc0504fc01fc00f900fb00fcfb04fb0508fe0b0d03"
    "f8f6ff0b0405fefb02f9ff030003fd0403f6fafc040202010406fdf604ff00fff9f70607060102fd00fefd01f80201fd0afe0202fbfe03fdf5f802fefe0801fc"
    "000df90b09fffe0902fd0b010200fe01fe030707070905fc06f6fc02f609faf7fbfb00ff06ff01fa03fbf408f9f9fb04f7fe040cfe00fb0cff0001fa00f809ff"
    "ff07f80909fb04ff0500fa04ff01060804f704fe07ff09030002f50401f9030202ff05050100fdfc04fdf70207fe0503fa02ff0407ff010508010403fc0a0501"
    "0703fd06000406060c01fffcfc0403fbfcfd0afa02f6ff09f807f501f900ff050201fd03fbfcfc040e000cfafd0304050aff070204ff08fa0006f90806ff0000"
    "000803f8fc00090100060402fcfe05000303020004050903fdfc04f7fd07fefcfd0609070402ff00f6fd04ff05f7fdfa07fffef9fdfafd0ef9fffb08fafb020a"
    "00000703ff080bfc0608fb04000707f3ff0903fafdf902f808050b07060604f400f602030109f906fa0304fdfb07fd08fd050501fe0307040904fcff010bfa02"
    "0907fffff5f6fb050508060501fb08feff02f90402fb02f804fd02fafbff05010705fbfe0306fbfcfa03fc0e050704fcf5fb05f3fd070701fe0204fefbfcfb00"
    "000404fff304fa0bfe0e040b0103fdfdfd05f906fe04fa00f5fcfffaff0101f3fefffbfa0c050607fafef501f4fc0503fafa0803fd0101f9fdf301010606fd0a"
    "fb06fdfcf8000e0103fe0304030900030a04fb0804fbfbfe0b01fc09fcfbff02000402ff03fbfa02f604fe0501fbfcfe0809ff01fb0902fcf8030c01fbfbfdf2"
    "02010906fdf501fc01f6fefff8f5f200f6010b020304f50909070202050203f3fffe03fb0605f900020007020afc0afe03f4fb070000f905fa0904fdfbfd0202"
    "f602f90bf406f9020703f9f609fb0507fa0103070606ffff01010806fffaf4ff00f4fe0201f7fcf709000107f4f909060c04fd05fd00fffb0d040102fcfe0102"
    "f701f506040605fe01fafd03f8fefd0603fd050c070101fafd0202f7f8f8f9fcfff9fcf4fe01fcf6fb01ff0100fbfafefcfc0201fd06fffe0501f602f6fe0104"
    "fafd040c0c050afcfe0505f607fafff9fe06f8fc00030a0107fc04f9f9f9fbfef50003f4f6f9fa0af8f502f50105fafbfa0804030500fc0205fffefa08050101"
    "020006010500fc07070afdfcf400fb07f906f8ff08fd020401030607f8fff302fc02f5f90304fefd04f6fdfa010d080102fffafc000701fef3fb0a01fe0a00f4"
    "fd0907fe0803070501fefe00050509ff02f4fcfc0001fd03fdfffbf808fb07fe0001fbf60501f6fcfc0703000703fbf7fc080507f7fe00fdfc0200fafcfe00fe"
)
DEFAULT_PATTERN = np.frombuffer(bytes.fromhex(_DEFAULT_PATTERN_HEX), np.int8).reshape(256, 4)
DEFAULT_PATTERN.flags.writeable = False


def level_sizes(H: int, W: int, n_levels: int = 8, scale: float = 1.2) -> Tuple[np.ndarray, np.ndarray]:
    """(heights, widths) int32 [L] = round(H / s^l), round(W / s^l): computed once here, handed to the library as arrays."""
    lh = np.asarray([int(np.rint(H / scale ** l)) for l in range(n_levels)], np.int32)
    lw = np.asarray([int(np.rint(W / scale ** l)) for l in range(n_levels)], np.int32)
    return np.maximum(lh, 1), np.maximum(lw, 1)


def level_quotas(n_features: int, n_levels: int = 8, scale: float = 1.2) -> np.ndarray:
    """ORB's geometric rule: n (1 - f) / (1 - f^L) f^l with f = 1 / s, rounded; the last level takes the remainder."""
    if n_levels == 1:
        return np.asarray([n_features], np.int32)
    f = 1.0 / scale
    want = n_features * (1.0 - f) / (1.0 - f ** n_levels)
    q, total = [], 0
    for _ in range(n_levels - 1):
        q.append(int(np.rint(want)))
        total += q[-1]
        want *= f
    q.append(max(n_features - total, 0))
    return np.asarray(q, np.int32)


def check_pattern(pattern) -> np.ndarray:
    """int8 [256, 4] or ValueError: shape, integer values, every point within radius 15."""
    p = np.asarray(DEFAULT_PATTERN if pattern is None else pattern)
    if p.shape != (256, 4):
        raise ValueError(f"pattern must have shape [256, 4] (ax, ay, bx, by), got {p.shape}")
    if not np.issubdtype(p.dtype, np.integer):
        raise ValueError(f"pattern must be an integer array, got {p.dtype}")
    p = p.astype(np.int64)
    if ((p[:, 0] ** 2 + p[:, 1] ** 2 > PATTERN_RADIUS ** 2) | (p[:, 2] ** 2 + p[:, 3] ** 2 > PATTERN_RADIUS ** 2)).any():
        raise ValueError(f"every pattern point must have norm <= {PATTERN_RADIUS}")
    return p.astype(np.int8)


def steered_table(pattern=None) -> np.ndarray:
    """int8 [32, 256, 4]: bins 0..7 are rint of the pattern turned by bin * 11.25 degrees, bins 8..31 exact quarter turns
    (x, y) -> (-y, x) of the bin 8 below, so the table is 4-fold symmetric."""
    p = check_pattern(pattern).astype(np.float64).reshape(256, 2, 2)
    t = np.zeros((N_BINS, 256, 2, 2), np.int64)
    for b in range(8):
        a = np.deg2rad(b * 360.0 / N_BINS)
        t[b, :, :, 0] = np.rint(np.cos(a) * p[:, :, 0] - np.sin(a) * p[:, :, 1])
        t[b, :, :, 1] = np.rint(np.sin(a) * p[:, :, 0] + np.cos(a) * p[:, :, 1])
    for b in range(8, N_BINS):
        t[b, :, :, 0] = -t[b - 8, :, :, 1]
        t[b, :, :, 1] = t[b - 8, :, :, 0]
    return np.ascontiguousarray(t.reshape(N_BINS, 256, 4).astype(np.int8))


def to_gray(img: np.ndarray) -> np.ndarray:
    """u8 [H, W] from a u8 [H, W] or [H, W, 3] image: (77 c0 + 150 c1 + 29 c2 + 128) >> 8 with c0 the FIRST channel (so an RGB
    image gets the Rec. 601 weights; a BGR image, as cv2.imread gives, should be reversed by the caller)."""
    a = np.asarray(img)
    if a.dtype != np.uint8:
        raise ValueError(f"images must be uint8, got {a.dtype}")
    if a.ndim == 3 and a.shape[2] == 3:
        c = a.astype(np.int32)
        return ((77 * c[:, :, 0] + 150 * c[:, :, 1] + 29 * c[:, :, 2] + 128) >> 8).astype(np.uint8)
    if a.ndim == 3 and a.shape[2] == 1:
        return np.ascontiguousarray(a[:, :, 0])
    if a.ndim != 2:
        raise ValueError(f"an image must be [H, W] or [H, W, 3], got shape {a.shape}")
    return a


class OrbParams:
    """Everything the library is told about one problem shape: validated sizes, level sizes, quotas, the steered table."""

    def __init__(self, H, W, n_features=500, n_levels=8, scale=1.2, fast_threshold=20, pattern=None, distribution="harris",
                 fast_threshold_min=None):
        for name, v in (("n_features", n_features), ("n_levels", n_levels), ("fast_threshold", fast_threshold)):
            if not isinstance(v, (int, np.integer)) or isinstance(v, bool):
                raise ValueError(f"{name} must be an integer")
        if not 1 <= n_levels <= MAX_LEVELS:
            raise ValueError(f"n_levels must be in [1, {MAX_LEVELS}]")
        if not 0 <= n_features <= MAX_FEATURES:
            raise ValueError(f"n_features must be in [0, {MAX_FEATURES}]")
        if not 1 <= fast_threshold <= 254:
            raise ValueError("fast_threshold must be in [1, 254]")
        if not (np.isfinite(scale) and 1.0 < scale <= 4.0):
            raise ValueError("scale must be in (1, 4]")
        if distribution not in DISTRIBUTIONS:
            raise ValueError(f"distribution must be one of {DISTRIBUTIONS}, got {distribution!r}")
        if fast_threshold_min is None:
            fast_threshold_min = fast_threshold
        if not isinstance(fast_threshold_min, (int, np.integer)) or isinstance(fast_threshold_min, bool):
            raise ValueError("fast_threshold_min must be an integer or None")
        if not 1 <= fast_threshold_min <= fast_threshold:
            raise ValueError("fast_threshold_min must be in [1, fast_threshold]")
        if distribution == "harris" and fast_threshold_min != fast_threshold:
            raise ValueError('fast_threshold_min below fast_threshold needs distribution="quadtree"')
        if not (1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE):
            raise ValueError(f"image sides must be in [1, {MAX_SIDE}], got {H} x {W}")
        self.H, self.W, self.L, self.scale, self.t = int(H), int(W), int(n_levels), float(scale), int(fast_threshold)
        self.lh, self.lw = level_sizes(H, W, n_levels, scale)
        self.quota = level_quotas(int(n_features), n_levels, scale)
        self.n_max = int(self.quota.sum())
        self.table = steered_table(pattern)
        self.distribution, self.t_min = distribution, int(fast_threshold_min)

    def workspace(self, B: int) -> Tuple[int, dict]:
        """(bytes, layout) of ``slam_orb_workspace``, or of ``slam_orb_dist_workspace`` for the quadtree mode: byte offsets of
        every stage buffer, so a test can download them."""
        n = ctypes.c_uint64(0)
        if self.distribution == "quadtree":
            lay = np.zeros(4 + 10 * self.L, np.uint64)
            check(load().slam_orb_dist_workspace(B, self.H, self.W, self.L, addr(self.lw), addr(self.lh), addr(self.quota), ctypes.byref(n),
                                                 addr(lay)))
            lv = lay[4:4 + 6 * self.L].reshape(self.L, 6).astype(np.int64)
            tree = lay[4 + 6 * self.L:].reshape(self.L, 4).astype(np.int64)
            return int(n.value), {"image_base": int(lay[0]), "image_stride": int(lay[1]), "counts": int(lay[2]), "selection": int(lay[3]),
                                  "image": lv[:, 0], "blur": lv[:, 1], "score": lv[:, 2], "candidates": lv[:, 3], "pitch": lv[:, 4],
                                  "capacity": lv[:, 5], "node_index": tree[:, 0], "nodes": tree[:, 1], "node_best": tree[:, 2],
                                  "node_capacity": tree[:, 3]}
        lay = np.zeros(4 + 6 * self.L, np.uint64)
        check(load().slam_orb_workspace(B, self.H, self.W, self.L, addr(self.lw), addr(self.lh), self.n_max, ctypes.byref(n), addr(lay)))
        lv = lay[4:].reshape(self.L, 6).astype(np.int64)
        return int(n.value), {"image_base": int(lay[0]), "image_stride": int(lay[1]), "counts": int(lay[2]), "selection": int(lay[3]),
                              "image": lv[:, 0], "blur": lv[:, 1], "score": lv[:, 2], "candidates": lv[:, 3], "pitch": lv[:, 4],
                              "capacity": lv[:, 5]}


class OrbResult:
    """The keypoints of a batch, per image ``b`` (rows ordered by level, then R descending, y, x):
    ``xy[b]`` f32 [n,2] level-0 pixels, ``level[b]``, ``bin[b]``, ``angle[b]`` (bin centre, degrees), ``response[b]`` (int64 R),
    ``size[b]`` (31 s^level), ``descriptors[b]`` u8 [n,32], ``xy_level[b]`` int32 [n,2] (level coordinates).
    With ``keep_on_device`` the descriptor block also stays resident: ``device_descriptors(b)``."""

    def __init__(self, params: OrbParams, count, kp, resp, desc, device_block: Optional[DeviceBuffer] = None):
        self.params, self.counts, self._block = params, count.astype(np.int64), device_block
        s = np.float32(params.scale) ** np.arange(params.L, dtype=np.float32)              # float32(s^l)
        self.xy_level, self.xy, self.level, self.bin, self.angle, self.response, self.size, self.descriptors = ([] for _ in range(8))
        for b, n in enumerate(self.counts):
            k = kp[b, :n]
            self.xy_level.append(np.ascontiguousarray(k[:, :2]))
            self.level.append(k[:, 2].copy())
            self.bin.append(k[:, 3].copy())
            self.xy.append(k[:, :2].astype(np.float32) * s[k[:, 2]][:, None])
            self.angle.append(k[:, 3].astype(np.float32) * np.float32(360.0 / N_BINS))
            self.size.append(np.float32(31.0) * s[k[:, 2]])
            self.response.append(resp[b, :n].copy())
            self.descriptors.append(np.ascontiguousarray(desc[b, :n]))

    def __len__(self):
        return len(self.counts)

    def device_descriptors(self, b: int) -> Tuple[DeviceBuffer, int]:
        """(device rows [n,32] of image ``b``, n): what ``knn2_device`` / ``ResidentMatcher`` take, no PCIe round trip."""
        if self._block is None:
            raise ValueError("the result was not made with keep_on_device=True")
        n = int(self.counts[b])
        return self._block.view(b * self.params.n_max * 32, n * 32), n

    def undistorted(self, camera, iterations: int = 10, ctx: Optional[Context] = None):
        """``Frame::UndistortKeyPoints``: (list of f64 [n,2] pinhole pixels per image, list of u8 [n] status) of ``xy`` under a
        ``CameraModel`` (``slamhip.camera``); NaN where the status is not 0."""
        from .camera import undistort_keypoints

        return undistort_keypoints(self, camera, iterations, ctx)

    def free(self) -> None:
        if self._block is not None:
            self._block.free()
            self._block = None


def _check_images(images, mask):
    a = np.asarray(images)
    if a.dtype != np.uint8:
        raise ValueError(f"images must be uint8, got {a.dtype}")
    if a.ndim == 2:
        a = a[None]
    if a.ndim != 3:
        raise ValueError(f"images must have shape [B, H, W] or [H, W], got {a.shape}")
    a = np.ascontiguousarray(a)
    m, batched = None, 0
    if mask is not None:
        m = np.asarray(mask)
        if m.dtype == np.bool_:
            m = m.astype(np.uint8)
        if m.dtype != np.uint8:
            raise ValueError(f"mask must be uint8 or bool, got {m.dtype}")
        if m.shape == a.shape[1:]:
            batched = 0
        elif m.shape == a.shape:
            batched = 1
        else:
            raise ValueError(f"mask shape {m.shape} matches neither [H, W] = {a.shape[1:]} nor [B, H, W] = {a.shape}")
        m = np.ascontiguousarray(m)
    return a, m, batched


def orb_extract_arrays(images, mask=None, n_features: int = 500, n_levels: int = 8, scale: float = 1.2, fast_threshold: int = 20,
                       pattern=None, ctx: Optional[Context] = None, keep_on_device: bool = False, distribution: str = "harris",
                       fast_threshold_min: Optional[int] = None) -> OrbResult:
    """ORB keypoints and descriptors of a batch of grayscale images u8 [B,H,W] (or one [H,W]); ``mask`` u8 [H,W] or [B,H,W],
    non-zero = allowed.  Arguments are validated here (ValueError) before the library is called.  ``distribution="quadtree"``
    spreads each level's quota by a quadtree and keeps corners down to ``fast_threshold_min`` (default: ``fast_threshold``) in
    cells that have none at ``fast_threshold``; it always runs on device-resident buffers."""
    a, m, batched = _check_images(images, mask)
    B, H, W = a.shape
    if H == 0 or W == 0:
        raise ValueError("images must not be empty")
    P = OrbParams(H, W, n_features, n_levels, scale, fast_threshold, pattern, distribution, fast_threshold_min)
    to_host = not keep_on_device and P.distribution == "harris"
    if B == 0 or to_host:
        count, kp = np.zeros(B, np.int32), np.zeros((B, P.n_max, 4), np.int32)
        resp, desc = np.zeros((B, P.n_max), np.int64), np.zeros((B, P.n_max, 32), np.uint8)
    if B == 0:
        return OrbResult(P, count, kp, resp, desc)
    ctx = ctx or default_context()
    if to_host:
        check(ctx.lib.slam_orb_extract_u8_host(ctx.handle, addr(a), B, H, W, addr(m) if m is not None else None, batched, P.L, addr(P.lw),
                                               addr(P.lh), addr(P.quota), P.t, addr(P.table), addr(count), addr(kp), addr(resp),
                                               addr(desc)))
        return OrbResult(P, count, kp, resp, desc)
    ex = OrbExtractor(ctx, B, P)
    try:
        ex.upload(a, m)
        ex.run()
        count, kp, resp, desc = ex.download()
        return OrbResult(P, count, kp, resp, desc, device_block=ex.release_descriptors() if keep_on_device else None)
    finally:
        ex.free()


class OrbExtractor:
    """Resident buffers for repeated extraction of one problem shape through ``slam_orb_extract_u8`` (the device entry), or
    through ``slam_orb_extract_dist_u8`` when the parameters ask for the quadtree distribution: images, optional mask, table,
    workspace and outputs stay on the device between calls."""

    def __init__(self, ctx: Context, B: int, params: OrbParams):
        self.ctx, self.B, self.P = ctx, int(B), params
        self.ws_bytes, self.layout = params.workspace(self.B)
        slots = max(self.B * params.n_max, 1)
        self.bufs = {"images": ctx.malloc(max(self.B * params.H * params.W, 16)), "table": ctx.upload(params.table),
                     "ws": ctx.malloc(self.ws_bytes), "count": ctx.malloc(max(4 * self.B, 16)), "kp": ctx.malloc(16 * slots),
                     "resp": ctx.malloc(8 * slots), "desc": ctx.malloc(32 * slots)}
        self.mask_batched = 0

    def upload(self, images: np.ndarray, mask: Optional[np.ndarray] = None) -> None:
        self.bufs["images"].upload(images)
        if mask is not None:
            if "mask" in self.bufs:
                self.bufs.pop("mask").free()
            self.bufs["mask"] = self.ctx.upload(mask)
            self.mask_batched = int(mask.ndim == 3)

    def upload_raw(self, images: np.ndarray, rect_map, border: int = 0, mask: Optional[np.ndarray] = None) -> None:
        """Raw (distorted) frames u8 [B, Hs, Ws] in, rectified frames in the resident image block: the frames are uploaded to a
        scratch buffer and resampled through ``rect_map`` (a ``slamhip.camera.RectifyMap`` of this extractor's W x H) on the
        device; the validity mask of the resampling becomes the detection mask.  The frames cross PCIe once.  With a caller's
        ``mask`` ([H, W] or [B, H, W], in rectified coordinates, non-zero = allowed) the validity mask is downloaded, ANDed
        with it on the host and uploaded again: one more round trip of B x H x W bytes."""
        from .camera import _check_border, _check_frames, remap_device

        a = _check_frames(images)
        border = _check_border(border)
        if rect_map.size != (self.P.W, self.P.H):
            raise ValueError(f"the map is {rect_map.size[0]} x {rect_map.size[1]}, the extractor {self.P.W} x {self.P.H}")
        if a.shape[0] != self.B:
            raise ValueError(f"{a.shape[0]} frames for an extractor of {self.B}")
        if rect_map.ctx is not self.ctx:
            raise ValueError("the map belongs to another context")
        m = None
        if mask is not None:
            m = np.asarray(mask)
            if m.dtype not in (np.uint8, np.bool_):
                raise ValueError(f"mask must be uint8 or bool, got {m.dtype}")
            if m.shape not in ((self.P.H, self.P.W), (self.B, self.P.H, self.P.W)):
                raise ValueError(f"mask shape {m.shape} matches neither [H, W] nor [B, H, W] of the extractor")
        if self.B == 0:
            return
        n = self.B * self.P.H * self.P.W
        if "mask" in self.bufs and (self.bufs["mask"].nbytes < n or not self.mask_batched):
            self.bufs.pop("mask").free()
        if "mask" not in self.bufs:
            self.bufs["mask"] = self.ctx.malloc(max(n, 16))
        self.mask_batched = 1
        raw = self.ctx.upload(a)
        try:
            remap_device(self.ctx, raw, self.B, a.shape[1], a.shape[2], rect_map, self.bufs["images"], self.bufs["mask"], border)
            if m is not None:
                valid = self.bufs["mask"].download(np.uint8, (self.B, self.P.H, self.P.W))
                self.bufs["mask"].upload(np.where((valid != 0) & (m != 0), 255, 0).astype(np.uint8))
            self.ctx.sync()
        finally:
            raw.free()

    def drop_mask(self) -> None:
        if "mask" in self.bufs:
            self.bufs.pop("mask").free()

    def run(self) -> None:
        P, b = self.P, self.bufs
        if P.distribution == "quadtree":
            check(self.ctx.lib.slam_orb_extract_dist_u8(self.ctx.handle, b["images"].ptr, self.B, P.H, P.W,
                                                        b["mask"].ptr if "mask" in b else None, self.mask_batched, P.L, addr(P.lw), addr(P.lh),
                                                        addr(P.quota), P.t, P.t_min, b["table"].ptr, b["ws"].ptr, self.ws_bytes,
                                                        b["count"].ptr, b["kp"].ptr, b["resp"].ptr, b["desc"].ptr))
            return
        check(self.ctx.lib.slam_orb_extract_u8(self.ctx.handle, b["images"].ptr, self.B, P.H, P.W, b["mask"].ptr if "mask" in b else None,
                                               self.mask_batched, P.L, addr(P.lw), addr(P.lh), addr(P.quota), P.t, b["table"].ptr, b["ws"].ptr,
                                               self.ws_bytes, b["count"].ptr, b["kp"].ptr, b["resp"].ptr, b["desc"].ptr))

    def download(self):
        P, b, B = self.P, self.bufs, self.B
        if P.n_max == 0:
            return (b["count"].download(np.int32, (B,)), np.zeros((B, 0, 4), np.int32), np.zeros((B, 0), np.int64),
                    np.zeros((B, 0, 32), np.uint8))
        return (b["count"].download(np.int32, (B,)), b["kp"].download(np.int32, (B, P.n_max, 4)),
                b["resp"].download(np.int64, (B, P.n_max)), b["desc"].download(np.uint8, (B, P.n_max, 32)))

    def stage(self, b: int, level: int):
        """Stage buffers of image ``b``, level ``level`` read back through the layout: (image, blurred, scores) u8 [h, w] and the
        candidate list as (R int64 [n], y, x)."""
        P, lay = self.P, self.layout
        h, w, pitch = int(P.lh[level]), int(P.lw[level]), int(lay["pitch"][level])
        base = lay["image_base"] + b * lay["image_stride"]
        planes = [self.bufs["ws"].view(base + int(lay[k][level]), pitch * h).download(np.uint8, (h, pitch))[:, :w] for k in ("image", "blur", "score")]
        n = int(self.bufs["ws"].view(lay["counts"] + 4 * (16 * b + level), 4).download(np.int32, (1,))[0])
        n = min(n, int(lay["capacity"][level]))
        if n == 0:                                            # an empty list may end the workspace: nothing to read
            raw = np.zeros((0, 2), np.int64)
        else:
            raw = self.bufs["ws"].view(base + int(lay["candidates"][level]), 16 * n).download(np.int64, (n, 2))
        xy = raw[:, 1] & 0xFFFFFFFF
        return planes[0], planes[1], planes[2], (raw[:, 0].copy(), (xy >> 16).astype(np.int64), (xy & 0xFFFF).astype(np.int64))

    def release_descriptors(self) -> DeviceBuffer:
        """Hands the descriptor block [B, N_max, 32] to the caller (who frees it); the extractor must not run again."""
        return self.bufs.pop("desc")

    def free(self) -> None:
        for v in self.bufs.values():
            v.free()
        self.bufs = {}


# ------------------------------------------------------------------------------------------------------ the drop-in detector
try:  # pragma: no cover - cv2 is absent on the build and GPU hosts
    from cv2 import KeyPoint as _CvKeyPoint
except Exception:  # noqa: BLE001
    _CvKeyPoint = None


class KeyPoint:
    """Stand-in for ``cv2.KeyPoint`` when cv2 is not importable (the ``MatchList`` precedent): the attributes the reference reads."""

    __slots__ = ("pt", "size", "angle", "response", "octave", "class_id")

    def __init__(self, x, y, size, angle=-1.0, response=0.0, octave=0, class_id=-1):
        self.pt, self.size, self.angle, self.response, self.octave, self.class_id = (float(x), float(y)), float(size), float(angle), float(response), int(octave), int(class_id)

    def __repr__(self):
        return f"KeyPoint(pt={self.pt}, size={self.size:.1f}, angle={self.angle:.2f}, response={self.response:.4g}, octave={self.octave})"


def _keypoints(res: OrbResult, b: int = 0) -> list:
    make = _CvKeyPoint if _CvKeyPoint is not None else KeyPoint
    return [make(float(x), float(y), float(s), float(a), float(r), int(o))
            for (x, y), s, a, r, o in zip(res.xy[b], res.size[b], res.angle[b], res.response[b], res.level[b])]


class OrbFeatureDetector:
    """Drop-in for the reference's ``OrbFeatureDetector`` (``feature_detectors.py:18-26``), to be passed to ``Frontend`` explicitly
    (``frontend.py:55-69`` takes the detector by injection).  Same signatures; keypoints are ``cv2.KeyPoint`` when cv2 imports,
    else the ``KeyPoint`` stand-in.  A 3-channel image is converted by ``to_gray``.  ``OrbFeatureDetector.quadtree(...)`` makes
    one that spreads its keypoints by a quadtree and keeps one resident extractor per image shape."""

    distribution, fast_threshold_min = "harris", None          # the constructor keeps the reference's signature: see quadtree()

    def __init__(self, n_features: int = 500) -> None:
        self.n_features = n_features
        self._extractors = {}                                  # quadtree mode: one resident extractor per image shape

    @classmethod
    def quadtree(cls, n_features: int = 500, fast_threshold_min: Optional[int] = None) -> "OrbFeatureDetector":
        """A detector of the quadtree mode: the quota of every level spread by a quadtree, corners down to
        ``fast_threshold_min`` (default: the FAST threshold itself) kept in cells that have none at the FAST threshold."""
        OrbParams(64, 64, n_features, distribution="quadtree", fast_threshold_min=fast_threshold_min)     # ValueError before anything runs
        det = cls(n_features)
        det.distribution, det.fast_threshold_min = "quadtree", fast_threshold_min
        return det

    def detect(self, img: np.ndarray, mask: np.ndarray = None) -> Sequence:
        return self.detect_and_compute(img, mask)[0]

    def detect_and_compute(self, img: np.ndarray, mask: np.ndarray = None) -> tuple:
        if self.distribution == "quadtree":
            res = self._quadtree(to_gray(img), mask)
        else:
            res = orb_extract_arrays(to_gray(img), mask=mask, n_features=self.n_features)
        return _keypoints(res, 0), res.descriptors[0]

    def _quadtree(self, gray: np.ndarray, mask) -> OrbResult:
        a, m, _ = _check_images(gray, mask)
        ex = self._extractors.get(a.shape[1:])
        if ex is None:
            P = OrbParams(a.shape[1], a.shape[2], self.n_features, distribution="quadtree", fast_threshold_min=self.fast_threshold_min)
            ex = self._extractors[a.shape[1:]] = OrbExtractor(default_context(), 1, P)
        if m is None:
            ex.drop_mask()
        ex.upload(a, m)
        ex.run()
        return OrbResult(ex.P, *ex.download())

    def free(self) -> None:
        """Releases the resident extractors of the quadtree mode."""
        for ex in self._extractors.values():
            ex.free()
        self._extractors = {}
