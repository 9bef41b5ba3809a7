"""The host twin of csrc/pnp.hip for the tests: tests/pnp_twin.cpp compiled with g++ (-O2 -ffp-contract=off, x86-64 baseline:
no FMA instructions) into a temporary directory on first use and loaded through ctypes; and the same file compiled a second
time with -fsanitize=address,undefined as a stand-alone program that reads a job file and writes a result file."""
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
SRC = os.path.join(HERE, "pnp_twin.cpp")
FLAGS = ["-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function"]
_dir = None
_lib = None
_san = None


def _tmp():
    global _dir
    if _dir is None:
        _dir = tempfile.mkdtemp(prefix="pnp_twin_")
        atexit.register(shutil.rmtree, _dir, True)
    return _dir


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def lib():
    global _lib
    if _lib is None:
        out = os.path.join(_tmp(), "libpnptwin.so")
        subprocess.check_call(["g++", *FLAGS, "-shared", SRC, "-o", out])
        _lib = ctypes.CDLL(out)
        _lib.pnpt_p3p.argtypes = [ctypes.c_int64] + [ctypes.c_void_p] * 4
        _lib.pnpt_draw_sample.argtypes = [ctypes.c_uint64, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
        _lib.pnpt_inlier.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_double] * 5 + [ctypes.c_void_p]
        _lib.pnpt_ransac.argtypes = ([ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_double] * 4 +
                                     [ctypes.c_int, ctypes.c_double, ctypes.c_uint64] + [ctypes.c_void_p] * 4)
    return _lib


def p3p(X, x):
    """(pose [S,4,3,4], nsol int32 [S]) for X [S,3,3], x [S,3,2] (normalised)."""
    X = np.ascontiguousarray(X, np.float64).reshape(-1, 3, 3)
    x = np.ascontiguousarray(x, np.float64).reshape(-1, 3, 2)
    S = len(X)
    pose, n = np.zeros((S, 4, 3, 4)), np.zeros(S, np.int32)
    if S:
        lib().pnpt_p3p(S, _p(X), _p(x), _p(pose), _p(n))
    return pose, n


def draw_sample(seed, h, n):
    idx = np.zeros(3, np.int32)
    lib().pnpt_draw_sample(seed & ((1 << 64) - 1), h, n, _p(idx))
    return idx.tolist()


def inlier(T, X, px, K, threshold):
    X, px = np.ascontiguousarray(X, np.float64).reshape(-1, 3), np.ascontiguousarray(px, np.float64).reshape(-1, 2)
    T = np.ascontiguousarray(T, np.float64).reshape(12)
    out = np.zeros(len(X), np.uint8)
    if len(X):
        lib().pnpt_inlier(_p(T), len(X), _p(X), _p(px), *[float(v) for v in K], float(threshold), _p(out))
    return out.astype(bool)


def ransac(X, px, K, H, threshold, seed, with_counts=False):
    """slam_pnp_ransac_f64 for one candidate: (pose [3,4], mask bool [n], stats int32 [4]) and, asked for, the exact count of
    every (hypothesis, solution) as int32 [H,4] (-1: no such solution)."""
    X, px = np.ascontiguousarray(X, np.float64).reshape(-1, 3), np.ascontiguousarray(px, np.float64).reshape(-1, 2)
    n = len(X)
    pose, mask, st = np.zeros(12), np.zeros(max(n, 1), np.uint8), np.zeros(4, np.int32)
    counts = np.zeros((H, 4), np.int32) if with_counts else None
    Xb, pb = (X, px) if n else (np.zeros((1, 3)), np.zeros((1, 2)))
    rc = lib().pnpt_ransac(n, _p(Xb), _p(pb), *[float(v) for v in K], int(H), float(threshold), seed & ((1 << 64) - 1), _p(pose), _p(mask),
                           _p(st), _p(counts) if with_counts else None)
    assert rc == 0
    res = (pose.reshape(3, 4), mask[:n].astype(bool), st)
    return res + (counts,) if with_counts else res


def san_program():
    """Path of the stand-alone twin built with AddressSanitizer and UndefinedBehaviorSanitizer (no recovery: a report ends it)."""
    global _san
    if _san is None:
        out = os.path.join(_tmp(), "pnp_twin_san")
        subprocess.check_call(["g++", *[f for f in FLAGS if f != "-fPIC"], "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-DPNP_TWIN_MAIN", SRC, "-o", out])
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


def san_p3p(X, x):
    X = np.ascontiguousarray(X, np.float64).reshape(-1, 3, 3)
    x = np.ascontiguousarray(x, np.float64).reshape(-1, 3, 2)
    S = len(X)
    data = _run_san(struct.pack("qq", 0, S) + X.tobytes() + x.tobytes(), S * (4 + 384))
    return np.frombuffer(data, np.float64, 48 * S, 4 * S).reshape(S, 4, 3, 4).copy(), np.frombuffer(data, np.int32, S).copy()


def san_ransac(X, px, K, H, threshold, seed):
    X, px = np.ascontiguousarray(X, np.float64).reshape(-1, 3), np.ascontiguousarray(px, np.float64).reshape(-1, 2)
    n = len(X)
    job = struct.pack("qqqQ5d", 1, n, H, seed & ((1 << 64) - 1), *[float(v) for v in K], float(threshold)) + X.tobytes() + px.tobytes()
    data = _run_san(job, 96 + 16 + n)
    return (np.frombuffer(data, np.float64, 12).reshape(3, 4).copy(), np.frombuffer(data, np.uint8, n, 112).astype(bool),
            np.frombuffer(data, np.int32, 4, 96).copy())
