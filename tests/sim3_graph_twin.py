"""The host twin of csrc/sim3_graph.hip for the tests: tests/sim3_graph_twin.cpp compiled with g++ (-O2 -ffp-contract=off,
x86-64 baseline: no FMA instructions) into a temporary directory on first use and loaded through ctypes; and the same file
compiled a second time with -fsanitize=address,undefined as a stand-alone program that reads a job file and writes a result
file.  The twin's sin / cos / atan2 / log / exp are the host library's: it agrees with the device by tolerance, not bit for bit."""
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
SRC = os.path.join(HERE, "sim3_graph_twin.cpp")
FLAGS = ["-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function"]
_dir = None
_lib = None
_san = None


def _tmp():
    global _dir
    if _dir is None:
        _dir = tempfile.mkdtemp(prefix="sim3_graph_twin_")
        atexit.register(shutil.rmtree, _dir, True)
    return _dir


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _c(a, shape):
    a = np.ascontiguousarray(a, np.float64).reshape(shape)
    return a if a.size else np.zeros((1,) + tuple(shape[1:]))


def lib():
    global _lib
    if _lib is None:
        out = os.path.join(_tmp(), "libsim3graphtwin.so")
        subprocess.check_call(["g++", *FLAGS, "-shared", SRC, "-o", out])
        _lib = ctypes.CDLL(out)
        _lib.s3gt_edges.argtypes = [ctypes.c_int64] + [ctypes.c_void_p] * 4 + [ctypes.c_double, ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 5
        _lib.s3gt_update.argtypes = [ctypes.c_int64] + [ctypes.c_void_p] * 3
        _lib.s3gt_inverse7.argtypes = [ctypes.c_int64] + [ctypes.c_void_p] * 3
    return _lib


def _edge_args(Si, Sj, Z, Om):
    n = len(np.asarray(Si).reshape(-1, 13))
    return n, _c(Si, (-1, 13)), _c(Sj, (-1, 13)), _c(Z, (-1, 13)), _c(Om, (-1, 49))


def edges(Si, Sj, Z, Om, huber=0.0, fix_scale=False, full=True):
    """Per edge: dict(rho [n], why int32 [n]) and, full, W [n,7,7], Di, Dj [n,35] (28 upper-triangle entries of the end's
    share of H_vv by rows, then its 7 of b)."""
    n, Si, Sj, Z, Om = _edge_args(Si, Sj, Z, Om)
    m = max(n, 1)
    rho, why, W, Di, Dj = np.zeros(m), np.zeros(m, np.int32), np.zeros((m, 7, 7)), np.zeros((m, 35)), np.zeros((m, 35))
    assert lib().s3gt_edges(n, _p(Si), _p(Sj), _p(Z), _p(Om), float(huber), int(bool(fix_scale)), int(bool(full)), _p(rho), _p(why), _p(W),
                            _p(Di), _p(Dj)) == 0
    out = dict(rho=rho[:n], why=why[:n])
    if full:
        out.update(W=W[:n], Di=Di[:n], Dj=Dj[:n])
    return out


def update(dx, S):
    dx, S = _c(dx, (-1, 7)), _c(S, (-1, 13))
    n = len(np.asarray(dx).reshape(-1, 7)) if np.asarray(dx).size else 0
    out = np.zeros((max(n, 1), 13))
    lib().s3gt_update(n, _p(dx), _p(S), _p(out))
    return out[:n]


def inverse7(A):
    n = np.asarray(A).size // 49
    A = _c(A, (-1, 49))
    Inv, ok = np.zeros((max(n, 1), 49)), np.zeros(max(n, 1), np.int32)
    lib().s3gt_inverse7(n, _p(A), _p(Inv), _p(ok))
    return Inv[:n].reshape(-1, 7, 7), ok[:n].astype(bool)


def full_blocks(D):
    """[n,35] -> (H share [n,7,7] symmetric, b share [n,7])"""
    D = np.asarray(D)
    H = np.zeros((len(D), 7, 7))
    iu = np.triu_indices(7)
    H[:, iu[0], iu[1]] = D[:, :28]
    H[:, iu[1], iu[0]] = D[:, :28]
    return H, D[:, 28:]


def san_program():
    """Path of the stand-alone twin built with AddressSanitizer and UndefinedBehaviorSanitizer (no recovery: a report ends it)."""
    global _san
    if _san is None:
        out = os.path.join(_tmp(), "sim3_graph_twin_san")
        subprocess.check_call(["g++", *[f for f in FLAGS if f != "-fPIC"], "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-DS3G_TWIN_MAIN", SRC, "-o", out])
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


def san_edges(Si, Sj, Z, Om, huber=0.0, fix_scale=False, full=True):
    n, Si, Sj, Z, Om = _edge_args(Si, Sj, Z, Om)
    job = struct.pack("qqqqd", 0, n, int(bool(fix_scale)), int(bool(full)), float(huber))
    job += b"".join(a[:n].tobytes() for a in (Si, Sj, Z, Om))
    data = _run_san(job, n * 12 + (n * 8 * (49 + 70) if full else 0))
    out = dict(rho=np.frombuffer(data, np.float64, n).copy(), why=np.frombuffer(data, np.int32, n, 8 * n).copy())
    if full:
        o = 12 * n
        out["W"] = np.frombuffer(data, np.float64, 49 * n, o).reshape(n, 7, 7).copy()
        out["Di"] = np.frombuffer(data, np.float64, 35 * n, o + 392 * n).reshape(n, 35).copy()
        out["Dj"] = np.frombuffer(data, np.float64, 35 * n, o + 672 * n).reshape(n, 35).copy()
    return out


def san_update(dx, S):
    dx, S = np.ascontiguousarray(dx, np.float64).reshape(-1, 7), np.ascontiguousarray(S, np.float64).reshape(-1, 13)
    n = len(dx)
    data = _run_san(struct.pack("qqqqd", 1, n, 0, 0, 0.0) + dx.tobytes() + S.tobytes(), 104 * n)
    return np.frombuffer(data, np.float64, 13 * n).reshape(n, 13).copy()


def san_inverse7(A):
    A = np.ascontiguousarray(A, np.float64).reshape(-1, 49)
    n = len(A)
    data = _run_san(struct.pack("qqqqd", 2, n, 0, 0, 0.0) + A.tobytes(), 396 * n)
    return np.frombuffer(data, np.float64, 49 * n).reshape(n, 7, 7).copy(), np.frombuffer(data, np.int32, n, 392 * n).astype(bool)
