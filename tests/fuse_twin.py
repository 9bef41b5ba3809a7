"""The host twin of csrc/fuse_point.h for the tests: tests/fuse_twin.cpp compiled with g++ (-O2 -ffp-contract=off, x86-64
baseline: no FMA instructions) into a temporary directory on first use - a stand-alone program that reads a job file and prints
its results - and the same file a second time with -fsanitize=address,undefined (no recovery: a report ends it)."""
from __future__ import annotations

import atexit
import os
import shutil
import struct
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "fuse_twin.cpp")
INC = os.path.join(os.path.dirname(HERE), "slam-experiments_amd", "csrc")
FLAGS = ["-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function", "-I", INC]
_dir = None
_prog = {}


def _tmp():
    global _dir
    if _dir is None:
        _dir = tempfile.mkdtemp(prefix="fuse_twin_")
        atexit.register(shutil.rmtree, _dir, True)
    return _dir


def program(san: bool = False) -> str:
    if san not in _prog:
        out = os.path.join(_tmp(), "fuse_twin_san" if san else "fuse_twin")
        extra = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if san else []
        subprocess.check_call(["g++", *FLAGS, *extra, SRC, "-o", out])
        _prog[san] = out
    return _prog[san]


def _run(job: bytes, san: bool) -> str:
    fd, path = tempfile.mkstemp(dir=_tmp())
    with os.fdopen(fd, "wb") as f:
        f.write(job)
    r = subprocess.run([program(san), path], capture_output=True, text=True)
    os.unlink(path)
    assert r.returncode == 0, f"twin failed ({r.returncode}):\n{r.stderr[-4000:]}"
    return r.stdout


def _bits(words):
    return np.array([int(w, 16) for w in words], np.uint64).view(np.float64)


def gates(xyz, A, Ow, th, camera, bounds, scale, scale2, rng=None, normal=None, level=None, cos2_limit=0.25, margins=(0.64, 1.44), san=False):
    """(status, u, v, lp) of fp_gates for the points xyz [n,3]."""
    xyz = np.ascontiguousarray(xyz, np.float64).reshape(-1, 3)
    n = len(xyz)
    s, s2 = np.zeros(16), np.zeros(16)
    s[:len(scale)], s2[:len(scale2)] = scale, scale2
    flags = (1 if rng is not None else 0) | (2 if normal is not None else 0) | (4 if level is not None else 0)
    job = struct.pack("qqqq", 0, n, flags, len(scale))
    job += np.concatenate([np.asarray(camera, np.float64), np.asarray(bounds, np.float64), [cos2_limit, th, margins[0], margins[1]],
                           np.asarray(A, np.float64).reshape(12), np.asarray(Ow, np.float64).reshape(3), s, s2]).astype(np.float64).tobytes()
    job += xyz.tobytes()
    for a, dt in ((rng, np.float64), (normal, np.float64), (level, np.int32)):
        if a is not None:
            job += np.ascontiguousarray(a, dt).tobytes()
    rows = [ln.split() for ln in _run(job, san).strip().splitlines()]
    assert len(rows) == n
    return (np.array([int(r[0]) for r in rows], np.int32), _bits([r[1] for r in rows]), _bits([r[2] for r in rows]),
            np.array([int(r[3]) for r in rows], np.int32))


def candidates(u, v, xy, lim, san=False):
    """bool [n]: fp_candidate of the rows at xy f32 [n,2] with their limits lim f64 [n]."""
    xy, lim = np.ascontiguousarray(xy, np.float32).reshape(-1, 2), np.ascontiguousarray(lim, np.float64).reshape(-1)
    job = struct.pack("qqdd", 1, len(xy), u, v) + xy.tobytes() + lim.tobytes()
    line = _run(job, san).split("\n")[0]
    return np.array([ch == "1" for ch in line[:len(xy)]], bool)


def medians(D, san=False):
    """(median int [n], chosen row) of the distance table D int [n,n] by fp_median and fp_choice_key."""
    D = np.ascontiguousarray(D, np.int32)
    n = len(D)
    out = [int(x) for x in _run(struct.pack("qq", 2, n) + D.tobytes(), san).split()]
    return np.array(out[:n], np.int64), out[n]


def normal_range(X, centres, ref, level, scale, san=False):
    """(normal f64 [3], range f64 [2]) of fp_view / fp_normal_range for the views from centres f64 [n,3], in that order."""
    O = np.ascontiguousarray(centres, np.float64).reshape(-1, 3)
    s = np.zeros(16)
    s[:len(scale)] = scale
    job = struct.pack("qqqqq", 3, len(O), ref, level, len(scale)) + np.asarray(X, np.float64).reshape(3).tobytes() + s.tobytes() + O.tobytes()
    v = _bits(_run(job, san).split()[:5])
    return v[:3].copy(), v[3:].copy()
