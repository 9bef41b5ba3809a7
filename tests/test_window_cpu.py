"""CPU suite for the window-constrained top-2 search (bf_window.hip): the planner without a device, argument checks made
before any context or library call, the entry points declared and bound, their refusal without a GPU, and the kernels in
the gfx950 code object."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
ENTRY_POINTS = ("slam_bf_window_knn_u256", "slam_bf_window_knn_u256_host", "slam_bf_window_plan_describe")
M_LIMIT = 1 << 23
SHAPES = [(0, 0), (0, 1), (1, 0), (1, 1), (600, 600), (65536, 65536), (1 << 20, 1 << 20), (5, M_LIMIT - 1), (1 << 28, 1000),
          (1, 2), (3, 17)]


@pytest.mark.parametrize("num_cu", [1, 80, 256])
@pytest.mark.parametrize("cells", [0, 1, 2, 1000, 1 << 20, 1 << 30])
def test_plan_invariants(built, num_cu, cells):
    import slamhip

    for n, m in SHAPES:
        p = slamhip.plan_describe_window(n, m, cells=cells, num_cu=num_cu)
        side = p["side"]
        assert 1 <= side <= 1024 and p["cells"] == side * side and p["tiles"] == side * side
        if cells:                                          # the cap holds, and nothing below it is wasted
            assert side * side <= max(cells, 1) and (side == 1024 or (side + 1) ** 2 > cells), (n, m, cells, p)
        else:                                              # about one cell per train row
            assert side == min(1024, max(1, int(np.ceil(np.sqrt(m))))), (m, p)
        assert p["queries_per_item"] == 64 and p["chunk"] == 1024 and p["tile_max"] == 16
        assert 1 <= p["blocks"] <= num_cu * 8
        # workspace: linear in the rows, plus the histograms of the grid - never N x M
        assert p["workspace_bytes"] <= 48 * m + 12 * n + 24 * side * side + (1 << 16), (n, m, p)
        assert p["workspace_bytes"] >= 48 * m + 12 * n
        for parts, length in ((p["scan_parts_cells"], 2 * side * side + 3), (p["scan_parts_items"], side * side + 2)):
            assert parts == (0 if length <= 16384 else -(-length // 4096)), (length, parts)


def test_plan_refuses_the_key_limit_and_bad_arguments(built):
    import slamhip
    from slamhip import _lib

    lib = _lib.load()
    plan = (ctypes.c_int64 * 10)()
    assert lib.slam_bf_window_plan_describe(256, 10, M_LIMIT - 1, 0, plan) == 0
    assert lib.slam_bf_window_plan_describe(256, 10, M_LIMIT, 0, plan) == _lib.SLAM_ERR_INVALID
    assert lib.slam_bf_window_plan_describe(256, 10, M_LIMIT + 1, 0, plan) == _lib.SLAM_ERR_INVALID
    assert lib.slam_bf_window_plan_describe(256, (1 << 28) + 1, 10, 0, plan) == _lib.SLAM_ERR_INVALID
    assert lib.slam_bf_window_plan_describe(0, 10, 10, 0, plan) == _lib.SLAM_ERR_INVALID
    assert lib.slam_bf_window_plan_describe(256, -1, 10, 0, plan) == _lib.SLAM_ERR_INVALID
    assert lib.slam_bf_window_plan_describe(256, 10, 10, -1, plan) == _lib.SLAM_ERR_INVALID
    assert lib.slam_bf_window_plan_describe(256, 10, 10, 0, None) == _lib.SLAM_ERR_INVALID
    with pytest.raises(slamhip.SlamHipError, match="2\\^23"):
        slamhip.plan_describe_window(1, M_LIMIT)


def test_search_refuses_the_key_limit_without_a_device(built):
    """M >= 2^23 is SLAM_ERR_INVALID with a message before anything touches a device (a null context would be refused
    too, so the check order is pinned through the message)."""
    from slamhip import _lib

    lib = _lib.load()
    for fn in (lib.slam_bf_window_knn_u256, lib.slam_bf_window_knn_u256_host):
        assert fn(None, None, 1, None, M_LIMIT, None, None, None, 1.0, 2, 0, None, None) == _lib.SLAM_ERR_INVALID
    ctx = ctypes.c_void_p(1)                                        # never dereferenced: the size check comes first
    rc = lib.slam_bf_window_knn_u256(ctx, None, 1, None, M_LIMIT, None, None, None, 1.0, 2, 0, None, None)
    assert rc == _lib.SLAM_ERR_INVALID
    assert b"2^23" in lib.slam_last_error()
    rc = lib.slam_bf_window_knn_u256_host(ctx, None, 1, None, 4, None, None, None, 1.0, 3, 0, None, None)
    assert rc == _lib.SLAM_ERR_INVALID
    assert b"k=3" in lib.slam_last_error()


def _no_context(monkeypatch):
    from slamhip import matching

    monkeypatch.setattr(matching, "default_context", lambda: (_ for _ in ()).throw(AssertionError("context made")))


def test_argument_validation_comes_first(built, monkeypatch):
    import slamhip

    _no_context(monkeypatch)
    q, t = np.zeros((4, 32), np.uint8), np.zeros((6, 32), np.uint8)
    qxy, txy = np.zeros((4, 2), np.float32), np.zeros((6, 2), np.float32)
    f = slamhip.window_match_arrays
    for k in (0, 3, -1, 2.0, True, "2", None):
        with pytest.raises(ValueError):
            f(q, t, qxy, txy, 1.0, k)
    for bad_q in (np.zeros((4, 3)), np.zeros((5, 2)), np.zeros((4, 2, 1)), np.zeros(8)):
        with pytest.raises(ValueError):
            f(q, t, bad_q, txy, 1.0)
    for bad_t in (np.zeros((6, 3)), np.zeros((2, 6)), np.zeros((0, 2))):
        with pytest.raises(ValueError):
            f(q, t, qxy, bad_t, 1.0)
    for bad in (np.array([["a", "b"]] * 4), np.zeros((4, 2), complex), np.zeros((4, 2), object)):
        with pytest.raises(TypeError):
            f(q, t, bad, txy, 1.0)
    for bad_r in (np.ones(5, np.float32), np.ones(4), np.ones((6, 1)), np.ones((1, 6))):   # per-row radius: exactly [M]
        with pytest.raises(ValueError):
            f(q, t, qxy, txy, bad_r)
    for bad_r in (None, "3", b"3", np.array(["3"] * 6), 1j):
        with pytest.raises(TypeError):
            f(q, t, qxy, txy, bad_r)
    with pytest.raises(ValueError):                                 # descriptors keep as_descriptors' checks
        f(np.zeros((4, 31), np.uint8), t, qxy, txy, 1.0)
    with pytest.raises(ValueError):
        f(q.astype(np.float32), t, qxy, txy, 1.0)
    with pytest.raises(ValueError):
        slamhip.window_match_filtered(t, q, txy, qxy, np.ones(4))   # (source order: the radius follows the source rows)
    from feature_matchers import BruteForceFeatureMatcher

    with pytest.raises(ValueError):
        BruteForceFeatureMatcher(6).match_in_windows(t, q, txy, qxy[:3], 1.0)


def test_radius_forms_and_coercion(built):
    from slamhip import matching

    assert matching._window_radius(3, 5) == (3.0, None)
    assert matching._window_radius(np.float64(2.5), 0) == (2.5, None)
    assert matching._window_radius(np.array(7.0), 2) == (7.0, None)
    r, rows = matching._window_radius(np.inf, 3)
    assert r == np.inf and rows is None
    r, rows = matching._window_radius([1, 2, 3], 3)
    assert rows.dtype == np.float32 and rows.tolist() == [1.0, 2.0, 3.0]
    r, rows = matching._window_radius(np.zeros(0), 0)
    assert rows.shape == (0,)
    xy = matching._window_xy(np.arange(8, dtype=np.int32).reshape(4, 2), 4, "xy")
    assert xy.dtype == np.float32 and xy.flags.c_contiguous and xy[3].tolist() == [6.0, 7.0]
    assert matching._window_xy(np.zeros((0,)), 0, "xy").shape == (0, 2)        # Frame data with no features


def test_every_window_entry_point_is_declared_and_bound(built):
    import slamhip
    from slamhip import _lib

    with open(os.path.join(ROOT, "include", "slamhip.h")) as f:
        header = f.read()
    for name in ENTRY_POINTS:
        assert f"SLAM_API int {name}(" in header
        assert name in _lib.SIGNATURES
        assert getattr(_lib.load(), name) is not None
    decl = header[header.index("slam_bf_window_knn_u256"):]
    assert "frontend.py:181-187" in header[:header.index("SLAM_API int slam_bf_window_knn_u256(")][-3000:]
    assert "utils.py:58-73" in header[:header.index("SLAM_API int slam_bf_window_knn_u256(")][-3000:]
    assert decl
    for name in ("window_knn_device", "window_match_arrays", "window_match_filtered", "plan_describe_window"):
        assert callable(getattr(slamhip, name))


def test_dropin_match_in_windows_signature(built):
    import feature_matchers as fm

    sig = inspect.signature(fm.BruteForceFeatureMatcher.match_in_windows)
    assert list(sig.parameters) == ["self", "source_descriptors", "query_descriptors", "source_xy", "query_xy", "radius",
                                    "dist_threshold"]
    assert sig.parameters["dist_threshold"].default is None
    # match() is untouched
    assert list(inspect.signature(fm.BruteForceFeatureMatcher.match).parameters) == [
        "self", "source_descriptors", "query_descriptors", "dist_threshold"]


def test_entry_points_fail_loudly_without_gpu(built):
    import slamhip

    if slamhip.device_count() > 0:
        pytest.skip("a GPU is visible here")
    from feature_matchers import BruteForceFeatureMatcher

    q, xy = np.zeros((4, 32), np.uint8), np.zeros((4, 2), np.float32)
    with pytest.raises(slamhip.SlamHipError):
        slamhip.window_match_arrays(q, q, xy, xy, 10.0)
    with pytest.raises(slamhip.SlamHipError):
        slamhip.window_match_arrays(q, q, xy, xy, np.ones(4), k=1)
    with pytest.raises(slamhip.SlamHipError):
        slamhip.window_match_filtered(q, q, xy, xy, 10.0)
    with pytest.raises(slamhip.SlamHipError):
        BruteForceFeatureMatcher(6).match_in_windows(q, q, xy, xy, 10.0, 30.0)


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
            names |= set(re.findall(r"(\S*win_\S*)\.kd\b", text))
    for k in ("win_bounds_kernel", "win_grid_kernel", "win_count_kernel", "win_scatter_kernel", "win_scan_kernel",
              "win_decode_kernel", "win_scan_block_kernelIiE", "win_scan_block_kernelIlE", "win_scan_sum_kernel",
              "win_scan_apply_kernel"):
        assert any(k in n for n in names), (k, sorted(names))
