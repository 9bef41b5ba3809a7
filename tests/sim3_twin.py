"""The host twin of csrc/sim3.hip for the tests: tests/sim3_twin.cpp compiled with g++ (-O2 -ffp-contract=off, x86-64 baseline:
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
SRC = os.path.join(HERE, "sim3_twin.cpp")
FLAGS = ["-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function"]
MASK64 = (1 << 64) - 1
_dir = None
_lib = None
_san = None


def _tmp():
    global _dir
    if _dir is None:
        _dir = tempfile.mkdtemp(prefix="sim3_twin_")
        atexit.register(shutil.rmtree, _dir, True)
    return _dir


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def lib():
    global _lib
    if _lib is None:
        out = os.path.join(_tmp(), "libsim3twin.so")
        subprocess.check_call(["g++", *FLAGS, "-shared", SRC, "-o", out])
        _lib = ctypes.CDLL(out)
        _lib.s3t_threepoint.argtypes = [ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
        _lib.s3t_draw_sample.argtypes = [ctypes.c_uint64, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
        _lib.s3t_inlier.argtypes = [ctypes.c_void_p, ctypes.c_int64] + [ctypes.c_void_p] * 3 + [ctypes.c_double] * 5 + [ctypes.c_void_p]
        _lib.s3t_ransac.argtypes = ([ctypes.c_int64] + [ctypes.c_void_p] * 3 + [ctypes.c_double] * 4 +
                                    [ctypes.c_int, ctypes.c_double, ctypes.c_int, ctypes.c_uint64] + [ctypes.c_void_p] * 4)
        _lib.s3t_refit.argtypes = [ctypes.c_int64] + [ctypes.c_void_p] * 3 + [ctypes.c_int] + [ctypes.c_void_p] * 2
    return _lib


def _pts(X1, X2):
    X1, X2 = np.ascontiguousarray(X1, np.float64).reshape(-1, 3), np.ascontiguousarray(X2, np.float64).reshape(-1, 3)
    assert len(X1) == len(X2)
    return X1, X2


def _sig(sigma2, n):
    if sigma2 is None:
        return None
    s = np.ascontiguousarray(sigma2, np.float64).reshape(-1, 2)
    assert len(s) == n
    return s if n else np.zeros((1, 2))


def split(model):
    """(s, R, t) of model [...,13]."""
    m = np.asarray(model)
    T = m[..., :12].reshape(m.shape[:-1] + (3, 4))
    return m[..., 12], T[..., :3], T[..., 3]


def threepoint(X1, X2, fix_scale=False):
    """(model [S,13], ok int32 [S]) for X1, X2 [S,3,3]."""
    X1 = np.ascontiguousarray(X1, np.float64).reshape(-1, 3, 3)
    X2 = np.ascontiguousarray(X2, np.float64).reshape(-1, 3, 3)
    S = len(X1)
    model, ok = np.zeros((S, 13)), np.zeros(S, np.int32)
    if S:
        lib().s3t_threepoint(S, _p(X1), _p(X2), int(bool(fix_scale)), _p(model), _p(ok))
    return model, ok


def draw_sample(seed, h, n):
    idx = np.zeros(3, np.int32)
    lib().s3t_draw_sample(seed & MASK64, h, n, _p(idx))
    return idx.tolist()


def inlier(model, X1, X2, K, chi2, sigma2=None):
    X1, X2 = _pts(X1, X2)
    model = np.ascontiguousarray(model, np.float64).reshape(13)
    out = np.zeros(len(X1), np.uint8)
    if len(X1):
        lib().s3t_inlier(_p(model), len(X1), _p(X1), _p(X2), _p(_sig(sigma2, len(X1))), *[float(v) for v in K], float(chi2), _p(out))
    return out.astype(bool)


def ransac(X1, X2, K, H, chi2, seed, sigma2=None, fix_scale=False, with_counts=False):
    """slam_sim3_ransac_f64 for one candidate: (model [13], mask bool [n], stats int32 [4]) and, asked for, the exact count of
    every hypothesis as int32 [H] (-1: no model)."""
    X1, X2 = _pts(X1, X2)
    n = len(X1)
    model, mask, st = np.zeros(13), np.zeros(max(n, 1), np.uint8), np.zeros(4, np.int32)
    counts = np.zeros(H, np.int32) if with_counts else None
    A, B = (X1, X2) if n else (np.zeros((1, 3)), np.zeros((1, 3)))
    rc = lib().s3t_ransac(n, _p(A), _p(B), _p(_sig(sigma2, n)), *[float(v) for v in K], int(H), float(chi2), int(bool(fix_scale)),
                          seed & MASK64, _p(model), _p(mask), _p(st), _p(counts))
    assert rc == 0
    res = (model, mask[:n].astype(bool), st)
    return res + (counts,) if with_counts else res


def refit(X1, X2, mask=None, fix_scale=False):
    """slam_sim3_refit_f64 for one candidate: (model [13], stats int32 [2] = {points used, ok})."""
    X1, X2 = _pts(X1, X2)
    n = len(X1)
    model, st = np.zeros(13), np.zeros(2, np.int32)
    A, B = (X1, X2) if n else (np.zeros((1, 3)), np.zeros((1, 3)))
    m = None if mask is None else np.ascontiguousarray(np.asarray(mask).reshape(-1).astype(bool), np.uint8)
    assert m is None or len(m) == n
    if m is not None and n == 0:
        m = np.zeros(1, np.uint8)
    assert lib().s3t_refit(n, _p(A), _p(B), _p(m), int(bool(fix_scale)), _p(model), _p(st)) == 0
    return model, st


def san_program():
    """Path of the stand-alone twin built with AddressSanitizer and UndefinedBehaviorSanitizer (no recovery: a report ends it)."""
    global _san
    if _san is None:
        out = os.path.join(_tmp(), "sim3_twin_san")
        subprocess.check_call(["g++", *[f for f in FLAGS if f != "-fPIC"], "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-DSIM3_TWIN_MAIN", SRC, "-o", out])
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


def san_threepoint(X1, X2, fix_scale=False):
    X1 = np.ascontiguousarray(X1, np.float64).reshape(-1, 3, 3)
    X2 = np.ascontiguousarray(X2, np.float64).reshape(-1, 3, 3)
    S = len(X1)
    data = _run_san(struct.pack("qqq", 0, S, int(bool(fix_scale))) + X1.tobytes() + X2.tobytes(), S * (4 + 104))
    return np.frombuffer(data, np.float64, 13 * S, 4 * S).reshape(S, 13).copy(), np.frombuffer(data, np.int32, S).copy()


def san_ransac(X1, X2, K, H, chi2, seed, sigma2=None, fix_scale=False):
    X1, X2 = _pts(X1, X2)
    n = len(X1)
    job = struct.pack("qqqQqq5d", 1, n, H, seed & MASK64, int(bool(fix_scale)), int(sigma2 is not None), *[float(v) for v in K], float(chi2))
    job += X1.tobytes() + X2.tobytes() + (b"" if sigma2 is None else np.ascontiguousarray(sigma2, np.float64).reshape(n, 2).tobytes())
    data = _run_san(job, 104 + 16 + n)
    return (np.frombuffer(data, np.float64, 13).copy(), np.frombuffer(data, np.uint8, n, 120).astype(bool),
            np.frombuffer(data, np.int32, 4, 104).copy())


def san_refit(X1, X2, mask=None, fix_scale=False):
    X1, X2 = _pts(X1, X2)
    n = len(X1)
    job = struct.pack("qqqq", 2, n, int(bool(fix_scale)), int(mask is not None)) + X1.tobytes() + X2.tobytes()
    job += b"" if mask is None else np.asarray(mask).reshape(n).astype(np.uint8).tobytes()
    data = _run_san(job, 104 + 8)
    return np.frombuffer(data, np.float64, 13).copy(), np.frombuffer(data, np.int32, 2, 104).copy()
