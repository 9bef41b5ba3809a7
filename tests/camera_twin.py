"""The host twin of csrc/camera.hip for the tests: tests/camera_twin.cpp (csrc/cam_model.h, the text the kernels run) compiled
with g++ (-O2 -ffp-contract=off, x86-64 baseline: no FMA instructions) into a temporary directory on first use and loaded
through ctypes; and the same file compiled a second time with -fsanitize=address,undefined as a stand-alone program that reads
a job file and writes a result file."""
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
SRC = os.path.join(HERE, "camera_twin.cpp")
FLAGS = ["-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function"]
_dir = None
_lib = None
_san = None


def _tmp():
    global _dir
    if _dir is None:
        _dir = tempfile.mkdtemp(prefix="camera_twin_")
        atexit.register(shutil.rmtree, _dir, True)
    return _dir


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def lib():
    global _lib
    if _lib is None:
        out = os.path.join(_tmp(), "libcameratwin.so")
        subprocess.check_call(["g++", *FLAGS, "-shared", SRC, "-o", out])
        _lib = ctypes.CDLL(out)
        V, I, L = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
        _lib.cam_tw_points.argtypes = [I, L, V, I, V, V, V, V]
        _lib.cam_tw_map.argtypes = [V, V, V, L, L, V]
    return _lib


def _px(px):
    p = np.ascontiguousarray(np.asarray(px, np.float64).reshape(-1, 2))
    return p, len(p)


def _points(op, record, px, iterations):
    p, n = _px(px)
    rec = np.ascontiguousarray(record, np.float64).reshape(16)
    out, norm, st = np.zeros((max(n, 1), 2)), np.zeros((max(n, 1), 2)), np.zeros(max(n, 1), np.uint8)
    src = p if n else np.zeros((1, 2))
    assert lib().cam_tw_points(op, n, _p(rec), int(iterations), _p(src), _p(out), _p(norm), _p(st)) == 0
    return out[:n], norm[:n], st[:n]


def undistort(record, px, iterations=10):
    """slam_cam_undistort_f64 for one set: (pinhole pixels [n,2], normalised [n,2], status u8 [n])."""
    return _points(0, record, px, iterations)


def distort(record, px):
    """slam_cam_distort_f64 for one set: (raw pixels [n,2], distorted normalised [n,2], status u8 [n])."""
    return _points(1, record, px, 0)


def rectify_map(record, size_out, new_K, R=None):
    """slam_cam_rectify_map: int32 [H, W, 2]."""
    W, H = size_out
    rec = np.ascontiguousarray(record, np.float64).reshape(16)
    k = np.ascontiguousarray(new_K, np.float64).reshape(4)
    r = None if R is None else np.ascontiguousarray(R, np.float64).reshape(9)
    out = np.zeros((H, W, 2), np.int32)
    assert lib().cam_tw_map(_p(rec), _p(r), _p(k), W, H, _p(out)) == 0
    return out


def trig(a):
    """(cam_atan(a), cam_tan(a)) of f64 [n]: tan is meant for [0, pi/2) only."""
    a = np.ascontiguousarray(a, np.float64).reshape(-1)
    at, tn = np.zeros(max(len(a), 1)), np.zeros(max(len(a), 1))
    lib().cam_tw_trig.argtypes = [ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    lib().cam_tw_trig(len(a), _p(a if len(a) else np.zeros(1)), _p(at), _p(tn))
    return at[:len(a)], tn[:len(a)]


def image_bounds(record, size, iterations=10):
    """The four-corner rule of ComputeImageBounds on the twin: (min_x, max_x, min_y, max_y)."""
    W, H = size
    c, _, st = undistort(record, [[0, 0], [W, 0], [0, H], [W, H]], iterations)
    assert not st.any()
    return (min(c[0, 0], c[2, 0]), max(c[1, 0], c[3, 0]), min(c[0, 1], c[1, 1]), max(c[2, 1], c[3, 1]))


def san_program():
    """Path of the stand-alone twin built with AddressSanitizer and UndefinedBehaviorSanitizer (no recovery: a report ends it)."""
    global _san
    if _san is None:
        out = os.path.join(_tmp(), "camera_twin_san")
        subprocess.check_call(["g++", *[f for f in FLAGS if f != "-fPIC"], "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-DCAMERA_TWIN_MAIN", SRC, "-o", out])
        _san = out
    return _san


def _san_run(op, n, Hd, iterations, record, R, new_K, payload, size):
    job = struct.pack("5q", op, n, Hd, int(iterations), int(R is not None))
    job += np.ascontiguousarray(record, np.float64).reshape(16).tobytes()
    job += (np.zeros(9) if R is None else np.ascontiguousarray(R, np.float64).reshape(9)).tobytes()
    job += (np.ones(4) if new_K is None else np.ascontiguousarray(new_K, np.float64).reshape(4)).tobytes() + payload
    d = tempfile.mkdtemp(dir=_tmp())
    jp, rp = os.path.join(d, "job"), os.path.join(d, "result")
    with open(jp, "wb") as f:
        f.write(job)
    r = subprocess.run([san_program(), jp, rp], capture_output=True, text=True)
    assert r.returncode == 0, f"sanitized twin failed ({r.returncode}):\n{r.stderr[-4000:]}"
    data = open(rp, "rb").read()
    assert len(data) == size, (len(data), size)
    return data


def san_points(op, record, px, iterations=10):
    """cam_tw_points through the sanitized program: the raw result bytes (out [n,2], norm [n,2], status [n])."""
    p, n = _px(px)
    return _san_run(op, n, 0, iterations, record, None, None, p.tobytes(), 33 * n)


def san_map(record, size_out, new_K, R=None):
    W, H = size_out
    return _san_run(2, W, H, 0, record, R, new_K, b"", 8 * W * H)
