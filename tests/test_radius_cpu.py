"""CPU suite for the radius search (BFMatcher.radiusMatch): the planner without a device, the mapping of max_distance to
the kernel's threshold (C and Python, as pure functions), the entry points declared and bound, their refusal without a
GPU, the kernels in the gfx950 code object, and parity with cv2.BFMatcher.radiusMatch where OpenCV is installed."""
import ctypes
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
WS_CAP = 64 << 20
ENTRY_POINTS = ("slam_bf_radius_u256", "slam_bf_radius_u256_host", "slam_bf_radius_threshold", "slam_bf_radius_plan_describe")


SHAPES = [(1, 1), (1, 1000), (200, 200), (4096, 4096), (8192, 65536), (65536, 65536), (4, 100_000), (1024, 300_000),
          (4096, 1 << 20), (4, (1 << 23) + 4096), (1 << 20, 1 << 16), (1 << 30, 1000), (1, 2**31 - 1), (3, 0), (0, 100)]


@pytest.mark.parametrize("num_cu", [1, 80, 256, 304])
def test_plan_invariants(built, num_cu):
    import slamhip

    for n, m in SHAPES:
        p = slamhip.plan_describe_radius(n, m, num_cu=num_cu)
        assert p["qblocks"] == (n + 255) // 256 and p["passes"] == 1 and p["resident"] == 8
        assert p["short_max"] == 4096 and p["bins"] == 257
        chunks, rows = p["chunks"], p["chunk"]
        assert chunks >= 1 and rows >= 16 and rows % 16 == 0
        if m:                                           # the chunks cover every train row - beyond 2^23 too - none empty
            assert (chunks - 1) * rows < m <= chunks * rows, (n, m, p)
        # (bytes, saturated at 2^31 - 1; beyond the cap only when one chunk's table is larger)
        assert p["workspace_bytes"] == min(chunks * n * 4, 2**31 - 1) and (p["workspace_bytes"] <= WS_CAP or chunks == 1), (n, m, p)
        slots = num_cu * p["resident"]
        assert chunks <= max(1, -(-slots // max(p["qblocks"], 1))), (n, m, p)
        if n and m >= 256 * slots and n * 4 * slots <= WS_CAP:     # a long train set fills the chip with one round of blocks
            assert p["qblocks"] * chunks >= min(num_cu, slots), (n, m, p)


def test_plan_rejects_bad_arguments(built):
    from slamhip import _lib

    lib = _lib.load()
    plan = (ctypes.c_int32 * 8)()
    assert lib.slam_bf_radius_plan_describe(0, 10, 10, plan) == _lib.SLAM_ERR_INVALID
    assert lib.slam_bf_radius_plan_describe(256, -1, 10, plan) == _lib.SLAM_ERR_INVALID
    assert lib.slam_bf_radius_plan_describe(256, 10, 2**31, plan) == _lib.SLAM_ERR_INVALID
    assert lib.slam_bf_radius_plan_describe(256, 10, 10, None) == _lib.SLAM_ERR_INVALID
    assert lib.slam_bf_radius_plan_describe(256, 10, 10, plan) == 0


def threshold_by_definition(r):
    """th such that d < th <=> (float32)d <= (float32)r for every integer d in [0, 256], found by trying them all"""
    with np.errstate(over="ignore"):
        r32 = np.float32(r)
    return sum(1 for d in range(257) if np.float32(d) <= r32)


CASES = [float("nan"), -float("inf"), -1e9, -1.0, -0.5, -1e-30, -0.0, 0.0, 1e-30, 0.5, 0.999, 1.0, 40.0, 64.5, 95.99, 96.0, 104.0,
         128.0, 254.5, 255.0, 255.5, 255.99999, 255.999999999, 256.0, 256.5, 1000.0, 1e9, 3.5e38, 1e300, float("inf")]


@pytest.mark.parametrize("r", CASES)
def test_threshold_mapping(built, r):
    import slamhip
    from slamhip import _lib

    th = slamhip.radius_threshold(r)
    assert th == threshold_by_definition(r), r
    assert _lib.load().slam_bf_radius_threshold(r) == th, r      # (the ABI takes a float, as cv2's maxDistance)
    assert 0 <= th <= 257
    if not math.isnan(r) and 0 <= r < 255:
        assert th == math.floor(r) + 1


def test_threshold_rejects_what_is_not_a_number(built, monkeypatch):
    import slamhip
    from slamhip import matching

    monkeypatch.setattr(matching, "default_context", lambda: (_ for _ in ()).throw(AssertionError("context made")))
    q = np.zeros((4, 32), np.uint8)
    for bad in (None, "10", b"10"):
        with pytest.raises((TypeError, ValueError)):
            slamhip.radius_threshold(bad)
        with pytest.raises((TypeError, ValueError)):
            slamhip.radius_match_arrays(q, q, bad)
        with pytest.raises((TypeError, ValueError)):
            slamhip.radius_match_collection(q, [q], bad)


def test_every_radius_entry_point_is_declared_and_bound(built):
    import slamhip
    from slamhip import _lib

    with open(os.path.join(ROOT, "include", "slamhip.h")) as f:
        header = f.read()
    for name in ENTRY_POINTS:
        assert f"SLAM_API int {name}(" in header
        assert name in _lib.SIGNATURES
        assert getattr(_lib.load(), name) is not None
    for name in ("radius_match_arrays", "radius_match_collection", "radius_device", "radius_threshold", "plan_describe_radius"):
        assert callable(getattr(slamhip, name))
    assert callable(slamhip.KeyframeDatabase.query_radius)


def test_dropin_radius_match_signature(built):
    import inspect

    import feature_matchers as fm

    sig = inspect.signature(fm.BruteForceFeatureMatcher.radius_match)
    assert list(sig.parameters) == ["self", "query_descriptors", "train_descriptors", "max_distance", "compact_result"]
    assert sig.parameters["compact_result"].default is False


def test_entry_points_fail_loudly_without_gpu(built):
    import slamhip

    if slamhip.device_count() > 0:
        pytest.skip("a GPU is visible here")
    from feature_matchers import BruteForceFeatureMatcher

    q = np.zeros((4, 32), np.uint8)
    with pytest.raises(slamhip.SlamHipError):
        slamhip.radius_match_arrays(q, q, 10.0)
    with pytest.raises(slamhip.SlamHipError):
        slamhip.radius_match_collection(q, [q, q], 10.0)
    with pytest.raises(slamhip.SlamHipError):
        BruteForceFeatureMatcher(6).radius_match(q, q, 10.0)
    with pytest.raises(slamhip.SlamHipError):
        slamhip.KeyframeDatabase()


def test_kernels_are_in_the_gfx950_code_object(built, tmp_path):
    if not os.path.exists(OBJDUMP):
        pytest.skip("llvm-objdump of the ROCm toolchain not found")
    from slamhip import _lib

    local = os.path.join(str(tmp_path), "lib.so")
    shutil.copy(_lib.LIB_PATH, local)
    subprocess.run([OBJDUMP, "--offloading", local], cwd=str(tmp_path), check=True, capture_output=True)
    names = set()
    for f in os.listdir(str(tmp_path)):
        if "gfx950" in f:
            text = subprocess.run([OBJDUMP, "-t", os.path.join(str(tmp_path), f)], check=True, capture_output=True, text=True).stdout
            names |= set(re.findall(r"(\S*bf_radius\S*)\.kd\b", text))
    for k in ("scan_kernelILb0E", "scan_kernelILb1E", "prefix_kernel", "blocks_kernel", "offsets_kernel", "sort_short_kernel",
              "sort_hist_kernel", "sort_scan_kernel", "sort_scatter_kernel"):
        assert any(k in n for n in names), (k, sorted(names))
    assert not any("bf_top2" in n for n in names)                 # (tests/test_isa_handoff_cpu.py pins every bf_top2 kernel)


def test_parity_with_opencv(built):
    cv2 = pytest.importorskip("cv2")
    import slamhip

    if slamhip.device_count() < 1:
        pytest.skip("no GPU visible")
    rng = np.random.default_rng(3)
    q = rng.integers(0, 256, (300, 32), dtype=np.uint8)
    t = rng.integers(0, 256, (500, 32), dtype=np.uint8)
    t[10] = t[20] = q[0]
    bf = cv2.BFMatcher(cv2.NORM_HAMMING)
    for r in (0.0, 90.0, 100.5, 256.0):
        want = bf.radiusMatch(q, t, r)
        off, idx, dist = slamhip.radius_match_arrays(q, t, r)
        for i, lst in enumerate(want):
            a, b = off[i], off[i + 1]
            assert {(m.trainIdx, int(m.distance)) for m in lst} == set(zip(idx[a:b].tolist(), dist[a:b].tolist())), (r, i)
            assert [m.distance for m in lst] == dist[a:b].astype(float).tolist(), (r, i)
