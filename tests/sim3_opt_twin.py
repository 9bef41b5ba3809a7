"""The host twin of csrc/sim3_opt.hip for the tests: tests/sim3_opt_twin.cpp compiled with g++ (-O2 -ffp-contract=off, x86-64
baseline: no FMA instructions) into a temporary directory on first use and loaded through ctypes; and the same file compiled
a second time with -fsanitize=address,undefined as a stand-alone program that reads a job file and writes a result file."""
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
SRC = os.path.join(HERE, "sim3_opt_twin.cpp")
FLAGS = ["-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function"]
ITERATIONS = (5, 10, 5)
_dir = None
_lib = None
_san = None


def _tmp():
    global _dir
    if _dir is None:
        _dir = tempfile.mkdtemp(prefix="sim3_opt_twin_")
        atexit.register(shutil.rmtree, _dir, True)
    return _dir


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def lib():
    global _lib
    if _lib is None:
        out = os.path.join(_tmp(), "libsim3opttwin.so")
        subprocess.check_call(["g++", *FLAGS, "-shared", SRC, "-o", out])
        _lib = ctypes.CDLL(out)
        V, D, I = ctypes.c_void_p, ctypes.c_double, ctypes.c_int
        _lib.s3o_pair.argtypes = [V, V, D, D, D, D, I, V, V, V, V]
        _lib.s3o_pair.restype = None
        _lib.s3o_retract.argtypes = [V, V, V]
        _lib.s3o_retract.restype = None
        _lib.s3o_linearize.argtypes = [ctypes.c_int64] + [V] * 7 + [D] * 5 + [I, V]
        _lib.s3o_optimize.argtypes = [ctypes.c_int64] + [V] * 6 + [D] * 5 + [I] * 5 + [V] * 5
    return _lib


def _arrays(X1, X2, px1, px2, sigma2):
    X1, X2 = np.ascontiguousarray(X1, np.float64).reshape(-1, 3), np.ascontiguousarray(X2, np.float64).reshape(-1, 3)
    px1, px2 = np.ascontiguousarray(px1, np.float64).reshape(-1, 2), np.ascontiguousarray(px2, np.float64).reshape(-1, 2)
    n = len(X1)
    assert len(X2) == n and len(px1) == n and len(px2) == n
    sg = None if sigma2 is None else np.ascontiguousarray(sigma2, np.float64).reshape(-1, 2)
    assert sg is None or len(sg) == n
    if n == 0:                                            # (a pointer to something: nothing is read through it)
        X1 = X2 = np.zeros((1, 3))
        px1 = px2 = np.zeros((1, 2))
        sg = None if sg is None else np.zeros((1, 2))
    return n, X1, X2, px1, px2, sg


def pair(model, p, K, fix_scale=False):
    """One pair p [12] at a model: (e [4] = (e2, e1), c [2] = (c1, c2), depth [2] = (z, wz), J [4,7])."""
    model, p = np.ascontiguousarray(model, np.float64).reshape(13), np.ascontiguousarray(p, np.float64).reshape(12)
    e, c, d, J = np.zeros(4), np.zeros(2), np.zeros(2), np.zeros((4, 7))
    lib().s3o_pair(_p(model), _p(p), *[float(v) for v in K], int(bool(fix_scale)), _p(e), _p(c), _p(d), _p(J))
    return e, c, d, J


def retract(model, x):
    model, x = np.ascontiguousarray(model, np.float64).reshape(13), np.ascontiguousarray(x, np.float64).reshape(7)
    out = np.zeros(13)
    lib().s3o_retract(_p(model), _p(x), _p(out))
    return out


def linearize(X1, X2, px1, px2, model, K, delta=0.0, sigma2=None, active=None, fix_scale=False):
    """The 36 sums (28 upper H row by row, 7 b, cost) in the header's order."""
    n, X1, X2, px1, px2, sg = _arrays(X1, X2, px1, px2, sigma2)
    model = np.ascontiguousarray(model, np.float64).reshape(13)
    act = None if active is None else np.ascontiguousarray(np.asarray(active).astype(bool), np.uint8)
    sums = np.zeros(36)
    assert lib().s3o_linearize(n, _p(X1), _p(X2), _p(px1), _p(px2), _p(sg), _p(act), _p(model), *[float(v) for v in K], float(delta),
                               int(bool(fix_scale)), _p(sums)) == 0
    return sums


def optimize(X1, X2, px1, px2, model, K, sigma2=None, th2=10.0, iterations=ITERATIONS, min_pairs=10, fix_scale=False, with_work=False):
    """slam_sim3_optimize_f64 for one candidate: (model [13], mask bool [n], chi2 [n,2], stats int32 [4]) and, asked for,
    work int64 [2] = {trials, linearisations}."""
    n, X1, X2, px1, px2, sg = _arrays(X1, X2, px1, px2, sigma2)
    model = np.ascontiguousarray(model, np.float64).reshape(13)
    out, mask, chi2, st, work = np.zeros(13), np.zeros(max(n, 1), np.uint8), np.zeros((max(n, 1), 2)), np.zeros(4, np.int32), np.zeros(2, np.int64)
    rc = lib().s3o_optimize(n, _p(X1), _p(X2), _p(px1), _p(px2), _p(sg), _p(model), *[float(v) for v in K], float(th2),
                            *[int(v) for v in iterations], int(min_pairs), int(bool(fix_scale)), _p(out), _p(mask), _p(chi2), _p(st), _p(work))
    assert rc == 0
    res = (out, mask[:n].astype(bool), chi2[:n], st)
    return res + (work,) if with_work else res


def san_program():
    """Path of the stand-alone twin built with AddressSanitizer and UndefinedBehaviorSanitizer (no recovery: a report ends it)."""
    global _san
    if _san is None:
        out = os.path.join(_tmp(), "sim3_opt_twin_san")
        subprocess.check_call(["g++", *[f for f in FLAGS if f != "-fPIC"], "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-DSIM3_OPT_TWIN_MAIN", SRC, "-o", out])
        _san = out
    return _san


def san_optimize(X1, X2, px1, px2, model, K, sigma2=None, th2=10.0, iterations=ITERATIONS, min_pairs=10, fix_scale=False):
    X1, X2 = np.ascontiguousarray(X1, np.float64).reshape(-1, 3), np.ascontiguousarray(X2, np.float64).reshape(-1, 3)
    n = len(X1)
    job = struct.pack("7q5d", n, int(sigma2 is not None), *[int(v) for v in iterations], int(min_pairs), int(bool(fix_scale)),
                      *[float(v) for v in K], float(th2))
    job += np.ascontiguousarray(model, np.float64).reshape(13).tobytes() + X1.tobytes() + X2.tobytes()
    job += np.ascontiguousarray(px1, np.float64).reshape(n, 2).tobytes() + np.ascontiguousarray(px2, np.float64).reshape(n, 2).tobytes()
    job += b"" if sigma2 is None else np.ascontiguousarray(sigma2, np.float64).reshape(n, 2).tobytes()
    d = tempfile.mkdtemp(dir=_tmp())
    jp, rp = os.path.join(d, "job"), os.path.join(d, "result")
    with open(jp, "wb") as f:
        f.write(job)
    r = subprocess.run([san_program(), jp, rp], capture_output=True, text=True)
    assert r.returncode == 0, f"sanitized twin failed ({r.returncode}):\n{r.stderr[-4000:]}"
    data = open(rp, "rb").read()
    assert len(data) == 104 + 16 + 17 * n, (len(data), n)
    return (np.frombuffer(data, np.float64, 13).copy(), np.frombuffer(data, np.uint8, n, 120 + 16 * n).astype(bool),
            np.frombuffer(data, np.float64, 2 * n, 120).reshape(n, 2).copy(), np.frombuffer(data, np.int32, 4, 104).copy())
