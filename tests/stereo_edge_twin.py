"""The host twin of csrc/stereo_edge.h for the tests: tests/stereo_edge_twin.cpp compiled with g++ (-O2 -ffp-contract=off,
x86-64 baseline: no FMA instructions) into a temporary directory on first use and loaded through ctypes; and the same file
compiled a second time with -fsanitize=address,undefined as a stand-alone program that reads a job file and writes a result
file.  No sanitizer is loaded into Python."""
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
SRC = os.path.join(HERE, "stereo_edge_twin.cpp")
FLAGS = ["-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function"]
KEYS = ("e", "Jpose", "Jpoint", "chi2", "w", "rho", "inlier")
_dir = None
_lib = None
_san = None


def _tmp():
    global _dir
    if _dir is None:
        _dir = tempfile.mkdtemp(prefix="stereo_edge_twin_")
        atexit.register(shutil.rmtree, _dir, True)
    return _dir


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def lib():
    global _lib
    if _lib is None:
        out = os.path.join(_tmp(), "libstereoedgetwin.so")
        subprocess.check_call(["g++", *FLAGS, "-shared", SRC, "-o", out])
        _lib = ctypes.CDLL(out)
        _lib.se_tw_edges.restype = ctypes.c_int64
        _lib.se_tw_edges.argtypes = [ctypes.c_int64] * 3 + [ctypes.c_void_p] * 14
    return _lib


def _args(T12, X, op, ol, meas3, info, cam, deltas, gates):
    T12 = np.ascontiguousarray(T12, np.float64).reshape(-1, 12)
    X = np.ascontiguousarray(X, np.float64).reshape(-1, 3)
    op, ol = np.ascontiguousarray(op, np.int32).reshape(-1), np.ascontiguousarray(ol, np.int32).reshape(-1)
    meas3 = np.ascontiguousarray(meas3, np.float64).reshape(-1, 3)
    info = np.ascontiguousarray(info, np.float64).reshape(-1)
    assert len(op) == len(ol) == len(meas3) == len(info)
    par = np.array([*cam, *deltas, *gates], np.float64)
    assert par.shape == (9,)
    return T12, X, op, ol, meas3, info, par


def edges(T12, X, op, ol, meas3, info, cam, deltas=(0.0, 0.0), gates=(5.991, 7.815)):
    """Every edge on the twin: dict(e [O,3], Jpose [O,3,6], Jpoint [O,3,3], chi2, w, rho [O], inlier bool [O], count)."""
    T12, X, op, ol, meas3, info, par = _args(T12, X, op, ol, meas3, info, cam, deltas, gates)
    O, m = len(op), max(len(op), 1)
    o = dict(e=np.zeros((m, 3)), Jpose=np.zeros((m, 3, 6)), Jpoint=np.zeros((m, 3, 3)), chi2=np.zeros(m), w=np.zeros(m), rho=np.zeros(m),
             inlier=np.zeros(m, np.uint8))
    pad = lambda a, n: a if a.size else np.zeros(n, a.dtype)  # noqa: E731  (an empty array has no address worth passing)
    count = lib().se_tw_edges(len(T12), len(X), O, _p(pad(T12, 12)), _p(pad(X, 3)), _p(pad(op, 1)), _p(pad(ol, 1)), _p(pad(meas3, 3)),
                              _p(pad(info, 1)), _p(par), *[_p(o[k]) for k in KEYS])
    out = {k: o[k][:O] for k in KEYS}
    out["inlier"] = out["inlier"].astype(bool)
    out["count"] = int(count)
    return out


def result_bytes(o) -> bytes:
    return b"".join(np.ascontiguousarray(o[k]).tobytes() for k in KEYS[:-1]) + o["inlier"].astype(np.uint8).tobytes() + struct.pack("q", o["count"])


def san_program():
    """Path of the stand-alone twin built with AddressSanitizer and UndefinedBehaviorSanitizer (no recovery: a report ends it)."""
    global _san
    if _san is None:
        out = os.path.join(_tmp(), "stereo_edge_twin_san")
        subprocess.check_call(["g++", *[f for f in FLAGS if f != "-fPIC"], "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-DSTEREO_EDGE_TWIN_MAIN", SRC, "-o", out])
        _san = out
    return _san


def san_edges(T12, X, op, ol, meas3, info, cam, deltas=(0.0, 0.0), gates=(5.991, 7.815)) -> bytes:
    """``edges`` through the sanitized program: the raw result bytes (``result_bytes`` of the same call)."""
    T12, X, op, ol, meas3, info, par = _args(T12, X, op, ol, meas3, info, cam, deltas, gates)
    job = struct.pack("3q", len(T12), len(X), len(op)) + b"".join(a.tobytes() for a in (par, T12, X, op, ol, meas3, info))
    d = tempfile.mkdtemp(dir=_tmp())
    jp, rp = os.path.join(d, "job"), os.path.join(d, "result")
    with open(jp, "wb") as f:
        f.write(job)
    r = subprocess.run([san_program(), jp, rp], capture_output=True, text=True)
    assert r.returncode == 0, f"sanitized twin failed ({r.returncode}):\n{r.stderr[-4000:]}"
    with open(rp, "rb") as f:
        return f.read()
