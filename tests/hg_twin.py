"""The host twin of csrc/homography.hip for the tests: tests/hg_twin.cpp compiled with g++ (-O2 -ffp-contract=off, x86-64
baseline: no FMA instructions) into a temporary directory on first use and loaded through ctypes; and the same file compiled a
second time with -fsanitize=address,undefined as a stand-alone program that reads a job file and writes a result file."""
from __future__ import annotations

import atexit
import ctypes
import os
import shutil
import struct
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hg_twin.cpp")
FLAGS = ["-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function"]
_dir = None
_lib = None
_san = None
_M64 = (1 << 64) - 1


def _tmp():
    global _dir
    if _dir is None:
        _dir = tempfile.mkdtemp(prefix="hg_twin_")
        atexit.register(shutil.rmtree, _dir, True)
    return _dir


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _px(a):
    return np.ascontiguousarray(a, np.float64).reshape(-1, 2)


def _some(a):
    return a if len(a) else np.zeros((1, 2))


def lib():
    global _lib
    if _lib is None:
        out = os.path.join(_tmp(), "libhgtwin.so")
        subprocess.check_call(["g++", *FLAGS, "-shared", SRC, "-o", out])
        _lib = ctypes.CDLL(out)
        V, D = ctypes.c_void_p, ctypes.c_double
        _lib.hgt_fourpoint.argtypes = [ctypes.c_int64, V, V, V, V]
        _lib.hgt_draw_sample.argtypes = [ctypes.c_uint64, ctypes.c_int, ctypes.c_int, V]
        _lib.hgt_inlier.argtypes = [V, ctypes.c_int64, V, V, D, V]
        _lib.hgt_ransac.argtypes = [ctypes.c_int64, V, V, ctypes.c_int, D, ctypes.c_uint64, V, V, V, V]
        _lib.hgt_decompose.argtypes = [ctypes.c_int64, V, V, D, D, D, D, V, V, D, V, V, V, V, V, V, V]
        _lib.hgt_model_score.argtypes = [ctypes.c_int64, V, V, D, D, D, D, V, V, D, V, V]
    return _lib


def fourpoint(p1, p2):
    """(H [S,9], ok int32 [S]) for p1, p2 [S,4,2]."""
    p1 = np.ascontiguousarray(p1, np.float64).reshape(-1, 4, 2)
    p2 = np.ascontiguousarray(p2, np.float64).reshape(-1, 4, 2)
    S = len(p1)
    H, ok = np.zeros((S, 9)), np.zeros(S, np.int32)
    if S:
        lib().hgt_fourpoint(S, _p(p1), _p(p2), _p(H), _p(ok))
    return H, ok


def draw_sample(seed, h, n):
    idx = np.zeros(4, np.int32)
    lib().hgt_draw_sample(seed & _M64, h, n, _p(idx))
    return idx.tolist()


def inlier(H, px1, px2, threshold):
    px1, px2 = _px(px1), _px(px2)
    H = np.ascontiguousarray(H, np.float64).reshape(9)
    out = np.zeros(len(px1), np.uint8)
    if len(px1):
        lib().hgt_inlier(_p(H), len(px1), _p(px1), _p(px2), float(threshold), _p(out))
    return out.astype(bool)


def ransac(px1, px2, H, threshold, seed, with_counts=False):
    """slam_hg_ransac_f64 for one pair: (H [9], mask bool [n], stats int32 [4]) and, asked for, the exact count of every
    hypothesis as int32 [H] (-1: no model)."""
    px1, px2 = _px(px1), _px(px2)
    n = len(px1)
    Hm, mask, st = np.zeros(9), np.zeros(max(n, 1), np.uint8), np.zeros(4, np.int32)
    counts = np.zeros(H, np.int32) if with_counts else None
    rc = lib().hgt_ransac(n, _p(_some(px1)), _p(_some(px2)), int(H), float(threshold), seed & _M64, _p(Hm), _p(mask), _p(st),
                          _p(counts) if with_counts else None)
    assert rc == 0
    res = (Hm, mask[:n].astype(bool), st)
    return res + (counts,) if with_counts else res


def decompose(px1, px2, K, H, inlier=None, distance_thresh=50.0):
    """slam_hg_decompose_f64 for one pair: dict(pose_all [4,3,4], normal_all [4,3], count int32 [4], pose [3,4], sv [3],
    good bool [n], stats int32 [4])."""
    px1, px2 = _px(px1), _px(px2)
    n = len(px1)
    H = np.ascontiguousarray(H, np.float64).reshape(9)
    inl = None if inlier is None else np.ascontiguousarray(np.asarray(inlier).astype(np.uint8).reshape(-1))
    if inl is not None and len(inl) == 0:
        inl = np.zeros(1, np.uint8)
    pa, na, cnt, pose, sv = np.zeros(48), np.zeros(12), np.zeros(4, np.int32), np.zeros(12), np.zeros(3)
    good, st = np.zeros(max(n, 1), np.uint8), np.zeros(4, np.int32)
    rc = lib().hgt_decompose(n, _p(_some(px1)), _p(_some(px2)), *[float(v) for v in K], _p(H), None if inl is None else _p(inl),
                             float(distance_thresh), _p(pa), _p(na), _p(cnt), _p(pose), _p(sv), _p(good), _p(st))
    assert rc == 0
    return dict(pose_all=pa.reshape(4, 3, 4), normal_all=na.reshape(4, 3), count=cnt, pose=pose.reshape(3, 4), sv=sv,
                good=good[:n].astype(bool), stats=st)


def model_score(px1, px2, K, H, E, sigma=1.0):
    """slam_hg_model_score_f64 for one pair: (score int64 [2], ratio)."""
    px1, px2 = _px(px1), _px(px2)
    H, E = np.ascontiguousarray(H, np.float64).reshape(9), np.ascontiguousarray(E, np.float64).reshape(9)
    score, ratio = np.zeros(2, np.int64), np.zeros(1)
    rc = lib().hgt_model_score(len(px1), _p(_some(px1)), _p(_some(px2)), *[float(v) for v in K], _p(H), _p(E), float(sigma), _p(score),
                               _p(ratio))
    assert rc == 0
    return score, float(ratio[0])


def san_program():
    """Path of the stand-alone twin built with AddressSanitizer and UndefinedBehaviorSanitizer (no recovery: a report ends it)."""
    global _san
    if _san is None:
        out = os.path.join(_tmp(), "hg_twin_san")
        subprocess.check_call(["g++", *[f for f in FLAGS if f != "-fPIC"], "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-DHG_TWIN_MAIN", SRC, "-o", out])
        _san = out
    return _san


def _run_san(job: bytes, nbytes: int) -> bytes:
    d = tempfile.mkdtemp(dir=_tmp())
    jp, rp = os.path.join(d, "job"), os.path.join(d, "result")
    with open(jp, "wb") as f:
        f.write(job)
    r = subprocess.run([san_program(), jp, rp], capture_output=True, text=True)
    assert r.returncode == 0, f"sanitized twin failed ({r.returncode}):\n{r.stderr[-4000:]}"
    data = open(rp, "rb").read()
    assert len(data) == nbytes, (len(data), nbytes)
    return data


def san_fourpoint(p1, p2):
    p1 = np.ascontiguousarray(p1, np.float64).reshape(-1, 4, 2)
    p2 = np.ascontiguousarray(p2, np.float64).reshape(-1, 4, 2)
    S = len(p1)
    data = _run_san(struct.pack("qq", 0, S) + p1.tobytes() + p2.tobytes(), S * (4 + 72))
    return np.frombuffer(data, np.float64, 9 * S, 4 * S).reshape(S, 9).copy(), np.frombuffer(data, np.int32, S).copy()


def san_pair(px1, px2, K, H, threshold, seed, E, distance_thresh=50.0, sigma=1.0):
    """The RANSAC, the decomposition of its winner on its inliers and the scores against E, in the sanitized program: the raw
    result bytes (layout in hg_twin.cpp) split into a dict."""
    px1, px2 = _px(px1), _px(px2)
    n = len(px1)
    E = np.ascontiguousarray(E, np.float64).reshape(9)
    job = (struct.pack("qqqQ7d", 1, n, H, seed & _M64, *[float(v) for v in K], float(threshold), float(distance_thresh), float(sigma))
           + E.tobytes() + px1.tobytes() + px2.tobytes())
    data = _run_san(job, 72 + 16 + n + 384 + 96 + 96 + 24 + 16 + 16 + n + 16 + 8)
    o = 0

    def take(dtype, count):
        nonlocal o
        a = np.frombuffer(data, dtype, count, o).copy()
        o += a.nbytes
        return a

    return dict(H=take(np.float64, 9), stats=take(np.int32, 4), mask=take(np.uint8, n).astype(bool), pose_all=take(np.float64, 48).reshape(4, 3, 4),
                normal_all=take(np.float64, 12).reshape(4, 3), pose=take(np.float64, 12).reshape(3, 4), sv=take(np.float64, 3),
                count=take(np.int32, 4), dstats=take(np.int32, 4), good=take(np.uint8, n).astype(bool), score=take(np.int64, 2),
                ratio=float(take(np.float64, 1)[0]))
