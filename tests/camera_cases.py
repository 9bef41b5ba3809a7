"""The cameras of the lens-distortion tests (tests/test_camera_cpu.py, tests/test_camera_gpu.py) and the point sets they share.
Plain numbers: nothing here imports the package."""
from __future__ import annotations

import collections

import numpy as np

Case = collections.namedtuple("Case", "name K model coeffs size")
MODEL_CODE = {"pinhole": 0, "radtan": 1, "equidistant": 2}

# EuRoC MAV cam0 (the intrinsics of bench.py and smoke()), its published radial-tangential coefficients, 752 x 480
EUROC = Case("euroc-cam0", (458.654, 457.296, 367.215, 248.375), "radtan", (-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05, 0.0), (752, 480))
# TUM-VI cam0, Kannala-Brandt with four coefficients, 512 x 512
TUMVI = Case("tumvi-cam0", (190.978, 190.978, 254.93, 254.93), "equidistant", (0.0034823894, 0.0007150348, -0.0020532361, 0.0002029367), (512, 512))
PINHOLE = Case("pinhole", (400.0, 410.0, 160.5, 119.25), "pinhole", (), (320, 240))
# a radtan model whose fold lies inside the frame: xd = x (1 - 0.6 r^2) stops growing at r^2 = 1 / 1.8
FOLD = Case("fold", (300.0, 300.0, 320.0, 240.0), "radtan", (-0.6, 0.0, 0.0, 0.0, 0.0), (640, 480))
CASES = (EUROC, TUMVI, PINHOLE, FOLD)
FOLD_R2 = 1.0 / 1.8                                    # the fold of FOLD in pinhole normalised coordinates
FOLD_RD = np.sqrt(FOLD_R2) * (1.0 - 0.6 * FOLD_R2)     # the largest distorted radius FOLD produces: sqrt(1/1.8) * 2/3


def record(case) -> np.ndarray:
    """f64 [16] = {fx, fy, cx, cy, model, k[0..7], 0, 0, 0} (include/slamhip.h)."""
    r = np.zeros(16)
    r[:4], r[4] = case.K, MODEL_CODE[case.model]
    r[5:5 + len(case.coeffs)] = case.coeffs
    return r


def grid(case, margin: float = 0.0, step: float = 8.0) -> np.ndarray:
    """Raw pixels f64 [n,2] on a lattice over the frame extended by ``margin`` on each side, both far edges included."""
    W, H = case.size
    xs = np.append(np.arange(-margin, W + margin, step), W + margin)
    ys = np.append(np.arange(-margin, H + margin, step), H + margin)
    return np.stack(np.meshgrid(xs, ys), -1).reshape(-1, 2).astype(np.float64)


def disc(case, radius: float, n: int, seed: int) -> np.ndarray:
    """n raw pixels whose DISTORTED normalised radius is uniform in [0, radius): a disc around the principal point."""
    rng = np.random.default_rng(seed)
    r, a = rng.uniform(0, radius, n), rng.uniform(0, 2 * np.pi, n)
    fx, fy, cx, cy = case.K
    return np.stack([fx * r * np.cos(a) + cx, fy * r * np.sin(a) + cy], -1)


def rot_y(angle: float) -> np.ndarray:
    c, s = np.cos(angle), np.sin(angle)
    return np.asarray([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])
