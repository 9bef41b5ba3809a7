"""CPU suite: pinned train sets (slam_bf_train_pin / _refresh / _unpin, DESIGN.md 3c "Pinned train sets") without a device - the
entry points in the header and the ABI table and their refusal of null arguments, the pinned routing rule restated in Python
against slam_bf_mx_feed_describe_pinned with the unpinned rule unmoved beside it, and on the recording stand-in of
tests/test_teardown_cpu.py: a sharded matcher pins its train set once when it is built, a step issues what it issued before,
and free() unpins before anything is freed."""
import ctypes
import os

import numpy as np
import pytest

import test_mx_feed_cpu as F                                    # the unpinned rule and its grid: one copy
import test_teardown_cpu as TD                                  # the recording stand-in: one copy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "slamhip.h")

GRID_N = (1, 500, 8192, 20000, 65535, 65536, 65537, 100000, 131072, 131073, 262144, 1 << 20)
GRID_M = (1, 16384, 40000, 65535, 65536, 65537, 100000, 131072, 199999, 200000, 200001, 1 << 20)


# ---- the ABI --------------------------------------------------------------------------------------------------------------

def test_the_entry_points_are_declared_and_refuse_null_arguments(built):
    from slamhip import _lib

    lib = _lib.load()
    header = open(HEADER).read()
    p, i64, i32p, i64p = ctypes.c_void_p, ctypes.c_int64, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64)
    want = {
        "slam_bf_train_pin": ("(slam_ctx* ctx, const void* d_train, int64_t M);", [p, p, i64]),
        "slam_bf_train_refresh": ("(slam_ctx* ctx, const void* d_train);", [p, p]),
        "slam_bf_train_unpin": ("(slam_ctx* ctx, const void* d_train);", [p, p]),
        "slam_bf_mx_feed_describe_pinned": ("(int feed, int64_t N, int64_t M, int32_t* h_feed);", [ctypes.c_int, i64, i64, i32p]),
        "slam_bf_mx_image_launches": ("(slam_ctx* ctx, int64_t* h_count);", [p, i64p]),
        "slam_bf_train_pins": ("(slam_ctx* ctx, int64_t* h_count);", [p, i64p]),
    }
    for name, (decl, args) in want.items():
        assert f"SLAM_API int {name}{decl}" in header, name
        assert _lib.SIGNATURES[name] == (ctypes.c_int, args) and hasattr(lib, name), name
    some = ctypes.c_void_p(0x1000)                              # never dereferenced: the null context is refused first
    n = ctypes.c_int64(0)
    for name, args in (("slam_bf_train_pin", (None, some, 128)), ("slam_bf_train_refresh", (None, some)),
                       ("slam_bf_train_unpin", (None, some)), ("slam_bf_mx_image_launches", (None, ctypes.byref(n))),
                       ("slam_bf_train_pins", (None, ctypes.byref(n))), ("slam_bf_mx_feed_describe_pinned", (0, 4096, 4096, None))):
        assert getattr(lib, name)(*args) == _lib.SLAM_ERR_INVALID == -1, name
        assert name.encode() in lib.slam_last_error(), (name, lib.slam_last_error())


def test_only_feeds_0_1_2_and_real_sizes_exist(built):
    import slamhip
    from slamhip._lib import SlamHipError

    for feed in (-1, 3, 1 << 20):
        with pytest.raises(SlamHipError):
            slamhip.mx_feed_describe_pinned(4096, 4096, feed)
    for n, m in ((0, 4096), (4096, 0), (-1, -1)):
        with pytest.raises(SlamHipError):
            slamhip.mx_feed_describe_pinned(n, m)


# ---- routing --------------------------------------------------------------------------------------------------------------

def pinned_rule(n, m):
    """DESIGN.md 3c "Pinned train sets": the shapes that feed 0 runs from the image of a pinned train set, among those the
    32x32x64 kernel runs - the unpinned box, widened to the box of the shapes that measured faster from a pinned image."""
    return 40000 <= n <= 131072 and 32768 <= m <= 200000


def test_the_pinned_rule_is_the_measured_box_and_contains_the_unpinned_one(built):
    import slamhip

    for n in GRID_N + (39999, 40000, 40001, 49152):             # ... and the pinned box's own edges
        for m in GRID_M + (32767, 32768, 32769):
            assert slamhip.mx_feed_describe_pinned(n, m, 0) == (2 if pinned_rule(n, m) else 1), (n, m)
            assert slamhip.mx_feed_describe_pinned(n, m, 1) == 1
            assert slamhip.mx_feed_describe_pinned(n, m, 2) == 2
            assert pinned_rule(n, m) or not F.rule(n, m), (n, m)   # pinning never takes the image away


def test_the_unpinned_rule_has_not_moved(built):
    import slamhip

    for n in GRID_N:
        for m in GRID_M:
            assert slamhip.mx_feed_describe(n, m, 0) == (2 if 65536 <= n <= 131072 and 65536 <= m <= 200000 else 1), (n, m)
            assert slamhip.mx_feed_describe(n, m, 1) == 1 and slamhip.mx_feed_describe(n, m, 2) == 2
    F.test_auto_takes_the_image_exactly_inside_the_measured_box(True)


# ---- the sharded matchers on the recording stand-in -----------------------------------------------------------------------

def _descriptors(log):
    return lambda c, rows: type("D", (), {"buf": TD._Buf(log, 32 * max(len(rows), 1), "descriptors"),
                                          "free": lambda self: log.append("free:descriptors")})()


@pytest.mark.parametrize("kind", ["query", "train"])
def test_a_sharded_matcher_pins_once_steps_as_before_and_unpins_before_it_frees(kind, monkeypatch):
    from slamhip import dist

    log = []
    ctx = TD._Ctx(log)
    monkeypatch.setattr(dist, "DeviceDescriptors", _descriptors(log))
    q, t = np.zeros((10, 32), np.uint8), np.zeros((20, 32), np.uint8)
    sm = dist.ShardedMatcher(ctx, 0, 1, q, t) if kind == "query" else dist.TrainShardedMatcher(ctx, 0, 1, q, t, 0)
    pins = [x for x in log if "train_pin" in x or "train_unpin" in x or "train_refresh" in x]
    assert pins == ["slam_bf_train_pin"]
    del log[:]
    for _ in range(3):
        sm.step()
    assert [x for x in log if x.startswith("slam_")] == ["slam_bf_knn2_u256"] * 3
    del log[:]
    sm.free()
    assert log.count("slam_bf_train_unpin") == 1 and "slam_bf_train_pin" not in log
    first_free = min(k for k, x in enumerate(log) if x.startswith("free:"))
    assert log.index("slam_bf_train_unpin") < first_free
    assert "free:descriptors" in log


def test_an_empty_train_set_is_not_pinned_and_a_broadcast_one_is_pinned_behind_a_wait(monkeypatch):
    from slamhip import dist

    log = []
    ctx = TD._Ctx(log)
    monkeypatch.setattr(dist, "DeviceDescriptors", lambda c, host=None, rows=None: _descriptors(log)(c, host if host is not None else range(rows)))
    q, t = np.zeros((10, 32), np.uint8), np.zeros((20, 32), np.uint8)
    sm = dist.ShardedMatcher(ctx, 0, 1, q, t[:0])
    assert "slam_bf_train_pin" not in log
    sm.free()
    assert "slam_bf_train_unpin" not in log
    del log[:]
    dist.ShardedMatcher(ctx, 1, 2, q, t, collective="rccl", broadcast_train=True)
    assert log.index("slam_comm_broadcast") < log.index("sync") < log.index("slam_bf_train_pin")
