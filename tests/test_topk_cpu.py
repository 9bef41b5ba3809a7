"""CPU suite for the top-k search (knnMatch with k up to 32): the planner's invariants (slam_bf_topk_plan_describe needs no
device), the Python-side rejection of k outside [1, 32] before any context or library call, and the hand-derived known
answers of tests/golden/kat_topk.json against both oracle twins."""
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KAT = os.path.join(ROOT, "tests", "golden", "kat_topk.json")
PASS = 1 << 23
WS_CAP = 64 << 20


def kat_cases():
    with open(KAT) as f:
        d = json.load(f)
    for c in d["cases"]:
        train = np.array(d["trains"][c["train"]], np.uint8).reshape(-1, 32)
        yield c["name"], c["k"], np.array(c["query"], np.uint8).reshape(-1, 32), train, c["idx"], c["dist"]


@pytest.mark.parametrize("name,k,query,train,idx,dist", list(kat_cases()), ids=lambda v: v if isinstance(v, str) else "")
def test_known_answers_against_both_oracles(built, name, k, query, train, idx, dist):
    from oracle import oracle

    for i, d in (oracle.bf_knn_c(query, train, k, threads=4), oracle.bf_knn_np(query, train, k)):
        assert i.tolist() == idx, name
        assert d.tolist() == dist, name


SHAPES = [(1, 1), (1, 1000), (200, 200), (257, 511), (4096, 4096), (8192, 65536), (65536, 65536), (4096, 1 << 20),
          (256, PASS + 4096), (1 << 20, 1 << 16), (1, 3 * PASS + 5), (3, 0), (0, 100)]


@pytest.mark.parametrize("num_cu", [1, 80, 256, 304])
@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 8, 9, 16, 17, 31, 32])
def test_plan_invariants(built, num_cu, k):
    import slamhip

    for n, m in SHAPES:
        p = slamhip.plan_describe_topk(n, m, k, num_cu=num_cu)
        assert p["K"] in (4, 8, 16, 32) and k <= p["K"] and (p["K"] == 4 or p["K"] // 2 < k), (n, m, k, p)
        assert p["qblocks"] == (n + 255) // 256
        assert p["passes"] == (m + PASS - 1) // PASS
        mp = min(m, PASS)
        chunks, rows = p["chunks"], p["chunk"]
        assert chunks >= 1 and rows >= 16 and rows % 16 == 0
        if mp:                                          # the chunks of a full pass cover its rows exactly, none empty
            assert (chunks - 1) * rows < mp <= chunks * rows, (n, m, k, p)
        # every pass (the last one may be shorter) fits in the chunks the workspace was sized for
        assert p["merge"] == (1 if chunks > 1 else 0)
        assert p["workspace_bytes"] == (chunks * n * k * 4 if chunks > 1 else 0)
        assert p["workspace_bytes"] <= WS_CAP, (n, m, k, p)
        # the grid fills the chip: one round of resident blocks, unless the rows or the workspace cap leave fewer chunks
        slots = num_cu * p["resident"]
        by_rows = -(-mp // 256)
        by_cap = WS_CAP // max(n * k * 4, 1)
        if n and mp:
            # (chunk rows are rounded up to whole groups of 16, which may cost a few chunks of a long train set)
            reachable = min(slots, p["qblocks"] * min(by_rows, max(by_cap, 1)))
            assert p["qblocks"] * chunks >= min(num_cu, reachable), (n, m, k, p)
            assert p["qblocks"] * chunks >= 0.98 * reachable, (n, m, k, p)
            assert chunks <= max(1, -(-slots // p["qblocks"])), (n, m, k, p)


def test_plan_resident_blocks_follow_the_register_budget(built):
    import slamhip

    # VGPRs of bf_topk_kernel<K> (DESIGN.md "Top-k search"): 63, 66, 74, 98 -> 8, 7, 6, 4 waves per SIMD
    assert [slamhip.plan_describe_topk(4096, 4096, k)["resident"] for k in (4, 8, 16, 32)] == [8, 7, 6, 4]


@pytest.mark.parametrize("k", [0, -1, 33, 64, 2.0, True, None, "3"])
def test_bad_k_is_rejected_before_any_library_call(built, monkeypatch, k):
    import slamhip
    from slamhip import _lib, device, matching

    def refuse(*a, **kw):
        raise AssertionError("a context or a library call was made before k was checked")

    monkeypatch.setattr(device, "default_context", refuse)
    monkeypatch.setattr(matching, "default_context", refuse)
    monkeypatch.setattr(matching, "load", refuse)
    monkeypatch.setattr(_lib, "load", refuse)
    q = np.zeros((4, 32), np.uint8)
    with pytest.raises(ValueError):
        slamhip.topk_match_arrays(q, q, k)
    with pytest.raises(ValueError):
        slamhip.topk_match_collection(q, [q, q], k)
    with pytest.raises(ValueError):
        slamhip.plan_describe_topk(4, 4, k)
    with pytest.raises(ValueError):
        slamhip.check_topk_k(k)


def test_top2_entry_points_keep_their_k_contract(built, monkeypatch):
    """knn_match_arrays and KeyframeDatabase.query still name the top-2 search: k outside {1, 2} is refused there."""
    import slamhip
    from slamhip import matching

    monkeypatch.setattr(matching, "default_context", lambda: (_ for _ in ()).throw(AssertionError("context made")))
    q = np.zeros((4, 32), np.uint8)
    for k in (0, 3, 5, 32):
        with pytest.raises(ValueError):
            slamhip.knn_match_arrays(q, q, k)
    db = object.__new__(slamhip.KeyframeDatabase)      # (no device buffer: the check comes first)
    with pytest.raises(ValueError):
        db.query(q, 3)


def test_every_topk_entry_point_is_declared_and_bound(built):
    from slamhip import _lib

    with open(os.path.join(ROOT, "include", "slamhip.h")) as f:
        header = f.read()
    assert "#define SLAM_BF_KNN_MAX 32" in header and _lib.BF_KNN_MAX == 32
    for name in ("slam_bf_knn_u256", "slam_bf_knn_u256_host", "slam_bf_merge_topk", "slam_bf_topk_plan_describe"):
        assert f"SLAM_API int {name}(" in header
        assert name in _lib.SIGNATURES
        assert getattr(_lib.load(), name) is not None


def test_describe_rejects_bad_arguments(built):
    import ctypes

    from slamhip import _lib

    lib = _lib.load()
    plan = (ctypes.c_int32 * 8)()
    assert lib.slam_bf_topk_plan_describe(256, 10, 10, 0, plan) == _lib.SLAM_ERR_INVALID
    assert lib.slam_bf_topk_plan_describe(256, 10, 10, 33, plan) == _lib.SLAM_ERR_INVALID
    assert lib.slam_bf_topk_plan_describe(0, 10, 10, 4, plan) == _lib.SLAM_ERR_INVALID
    assert lib.slam_bf_topk_plan_describe(256, -1, 10, 4, plan) == _lib.SLAM_ERR_INVALID
    assert lib.slam_bf_topk_plan_describe(256, 10, 10, 4, None) == _lib.SLAM_ERR_INVALID
    assert lib.slam_bf_topk_plan_describe(256, 10, 10, 4, plan) == 0
