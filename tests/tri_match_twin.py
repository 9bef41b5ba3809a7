"""The host twin of csrc/tri_point.h for the tests: tests/tri_match_twin.cpp compiled with g++ (-O2 -ffp-contract=off, x86-64
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
SRC = os.path.join(HERE, "tri_match_twin.cpp")
INC = os.path.join(os.path.dirname(HERE), "slam-experiments_amd", "csrc")
FLAGS = ["-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function", "-I", INC]
_dir = None
_prog = {}


def _tmp():
    global _dir
    if _dir is None:
        _dir = tempfile.mkdtemp(prefix="tri_twin_")
        atexit.register(shutil.rmtree, _dir, True)
    return _dir


def program(san: bool = False) -> str:
    if san not in _prog:
        out = os.path.join(_tmp(), "tri_match_twin_san" if san else "tri_match_twin")
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


def _head(mode, scale, sigma2):
    s, s2 = np.zeros(16), np.zeros(16)
    s[:len(scale)], s2[:len(sigma2)] = scale, sigma2
    return struct.pack("qq", mode, len(scale)) + s.tobytes() + s2.tobytes()


def gates(F, epipole, xy1, xy2, level2, scale, sigma2, chi2=3.84, epipole_r2=100.0, san=False):
    """(off_epipole bool [n1, n2], on_line bool [n1, n2]) from tp_off_epipole / tp_on_line."""
    xy1, xy2 = np.ascontiguousarray(xy1, np.float32).reshape(-1, 2), np.ascontiguousarray(xy2, np.float32).reshape(-1, 2)
    lv = np.ascontiguousarray(level2, np.int32).reshape(-1)
    num = np.concatenate([[chi2, epipole_r2], np.asarray(F, np.float64).reshape(9), np.asarray(epipole, np.float64).reshape(2)])
    job = _head(0, scale, sigma2) + num.tobytes() + struct.pack("qq", len(xy1), len(xy2)) + xy1.tobytes() + xy2.tobytes() + lv.tobytes()
    lines = _run(job, san).split("\n")[:len(xy1)]
    code = np.array([[ord(ch) - 48 for ch in ln] for ln in lines], np.int64).reshape(len(xy1), len(xy2))
    return (code & 1) != 0, (code & 2) != 0


def triangulate(T1, T2, camera, scale, sigma2, xy1, xy2, l1, l2, cos_max=0.9998, chi2_px=5.991, ratio_factor=None, san=False):
    """tp_triangulate for n matches (row k of xy1 with row k of xy2) -> dict status int32 [n], X, normal [n,3], dmin2, dmax2."""
    T1, T2 = np.ascontiguousarray(np.asarray(T1, np.float64)[:3]), np.ascontiguousarray(np.asarray(T2, np.float64)[:3])
    O1, O2 = -T1[:, :3].T @ T1[:, 3], -T2[:, :3].T @ T2[:, 3]
    return triangulate_centres(T1, T2, O1, O2, camera, scale, sigma2, xy1, xy2, l1, l2, cos_max, chi2_px, ratio_factor, san)


def triangulate_centres(T1, T2, O1, O2, camera, scale, sigma2, xy1, xy2, l1, l2, cos_max=0.9998, chi2_px=5.991, ratio_factor=None,
                        san=False):
    xy1, xy2 = np.ascontiguousarray(xy1, np.float32).reshape(-1, 2), np.ascontiguousarray(xy2, np.float32).reshape(-1, 2)
    l1, l2 = np.ascontiguousarray(l1, np.int32).reshape(-1), np.ascontiguousarray(l2, np.int32).reshape(-1)
    n = len(xy1)
    rf = 1.5 * (scale[1] if len(scale) > 1 else 1.0) if ratio_factor is None else ratio_factor
    num = np.concatenate([np.asarray(camera, np.float64), [cos_max, chi2_px, rf], np.asarray(T1, np.float64).reshape(12),
                          np.asarray(T2, np.float64).reshape(12), np.asarray(O1, np.float64), np.asarray(O2, np.float64)])
    job = _head(1, scale, sigma2) + num.tobytes() + struct.pack("q", n) + xy1.tobytes() + xy2.tobytes() + l1.tobytes() + l2.tobytes()
    st, val = np.zeros(n, np.int32), np.zeros((n, 8), np.uint64)
    for i, ln in enumerate(_run(job, san).split("\n")[:n]):
        parts = ln.split()
        st[i] = int(parts[0])
        val[i] = [int(p, 16) for p in parts[1:]]
    v = val.view(np.float64)
    return dict(status=st, X=v[:, 0:3].copy(), normal=v[:, 3:6].copy(), dmin2=v[:, 6].copy(), dmax2=v[:, 7].copy())
