"""The host twin of csrc/stereo.hip for the tests: tests/stereo_twin.cpp (csrc/stereo_point.h, the text the kernels run) compiled
with g++ (-O2 -ffp-contract=off, x86-64 baseline: no FMA instructions) into a temporary directory on first use and loaded
through ctypes; and the same file compiled a second time with -fsanitize=address,undefined as a stand-alone program that reads
a job file and writes a result file.  No sanitizer is loaded into Python."""
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
SRC = os.path.join(HERE, "stereo_twin.cpp")
FLAGS = ["-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function"]
KEYS = ("right", "u_right", "depth", "orb_dist", "sad", "status")
_dir = None
_lib = None
_san = None


def _tmp():
    global _dir
    if _dir is None:
        _dir = tempfile.mkdtemp(prefix="stereo_twin_")
        atexit.register(shutil.rmtree, _dir, True)
    return _dir


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def lib():
    global _lib
    if _lib is None:
        out = os.path.join(_tmp(), "libstereotwin.so")
        subprocess.check_call(["g++", *FLAGS, "-shared", SRC, "-o", out])
        _lib = ctypes.CDLL(out)
        V, I, L, D = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_double
        _lib.st_tw_pair.argtypes = [L, V, V, V, L, V, V, V, I, V, V, V, V, V, D, D, D, I, I, I, I, V, V, V, V, V, V, V]
    return _lib


def pack(planes):
    """The levels of one image as one dense buffer: (bytes u8 [n], off uint64 [16], pitch, w, h int32 [16])."""
    off, pitch, lw, lh = np.zeros(16, np.uint64), np.ones(16, np.int32), np.ones(16, np.int32), np.ones(16, np.int32)
    parts, at = [], 0
    for l, pl in enumerate(planes):
        h, w = pl.shape
        off[l], pitch[l], lw[l], lh[l] = at, w, w, h
        parts.append(np.ascontiguousarray(pl, np.uint8).reshape(-1))
        at += h * w
    return (np.concatenate(parts) if parts else np.zeros(0, np.uint8)), off, pitch, lw, lh


def _args(kpL, descL, planesL, kpR, descR, planesR, scale):
    kpL, kpR = (np.ascontiguousarray(np.asarray(k, np.int32).reshape(-1, 4)) for k in (kpL, kpR))
    descL, descR = (np.ascontiguousarray(np.asarray(d, np.uint8).reshape(-1, 32)) for d in (descL, descR))
    imgL, off, pitch, lw, lh = pack(planesL)
    imgR = pack(planesR)[0]
    assert imgL.shape == imgR.shape, "the two pyramids must have one shape"
    sc = np.ones(16, np.float32)
    sc[:len(scale)] = scale
    return kpL, descL, imgL, kpR, descR, imgR, off, pitch, lw, lh, sc


def match_pair(kpL, descL, planesL, kpR, descR, planesR, scale, bf, max_d, min_d=0.0, th_orb=75, w=5, Ls=5, reject=True):
    """One pair on the twin: the dict ``stereo_ref.match_pair`` returns."""
    kpL, descL, imgL, kpR, descR, imgR, off, pitch, lw, lh, sc = _args(kpL, descL, planesL, kpR, descR, planesR, scale)
    nL, nR = len(kpL), len(kpR)
    m = max(nL, 1)
    o = dict(right=np.zeros(m, np.int32), u_right=np.zeros(m), depth=np.zeros(m), orb_dist=np.zeros(m, np.int32), sad=np.zeros(m, np.int32),
             status=np.zeros(m, np.uint8))
    counts = np.zeros(2, np.int32)
    pad = lambda a, n: a if len(a) else np.zeros(n, a.dtype)  # noqa: E731  (an empty array has no address worth passing)
    rc = lib().st_tw_pair(nL, _p(pad(kpL, 4)), _p(pad(descL, 32)), _p(pad(imgL, 1)), nR, _p(pad(kpR, 4)), _p(pad(descR, 32)), _p(pad(imgR, 1)),
                          len(scale), _p(off), _p(pitch), _p(lw), _p(lh), _p(sc), float(bf), float(min_d), float(max_d), int(th_orb), int(w), int(Ls),
                          int(bool(reject)), *[_p(o[k]) for k in KEYS], _p(counts))
    assert rc == 0
    out = {k: o[k][:nL] for k in KEYS}
    out["counts"] = counts
    return out


def san_program():
    """Path of the stand-alone twin built with AddressSanitizer and UndefinedBehaviorSanitizer (no recovery: a report ends it)."""
    global _san
    if _san is None:
        out = os.path.join(_tmp(), "stereo_twin_san")
        subprocess.check_call(["g++", *[f for f in FLAGS if f != "-fPIC"], "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-DSTEREO_TWIN_MAIN", SRC, "-o", out])
        _san = out
    return _san


def san_pair(kpL, descL, planesL, kpR, descR, planesR, scale, bf, max_d, min_d=0.0, th_orb=75, w=5, Ls=5, reject=True) -> bytes:
    """``match_pair`` through the sanitized program: the raw result bytes (the six arrays in ``KEYS`` order, then counts)."""
    kpL, descL, imgL, kpR, descR, imgR, off, pitch, lw, lh, sc = _args(kpL, descL, planesL, kpR, descR, planesR, scale)
    job = struct.pack("8q3d", len(kpL), len(kpR), len(scale), int(th_orb), int(w), int(Ls), int(bool(reject)), len(imgL), float(bf), float(min_d),
                      float(max_d))
    job += b"".join(a.tobytes() for a in (off, pitch, lw, lh, sc, kpL, descL, imgL, kpR, descR, imgR))
    d = tempfile.mkdtemp(dir=_tmp())
    jp, rp = os.path.join(d, "job"), os.path.join(d, "result")
    with open(jp, "wb") as f:
        f.write(job)
    r = subprocess.run([san_program(), jp, rp], capture_output=True, text=True)
    assert r.returncode == 0, f"sanitized twin failed ({r.returncode}):\n{r.stderr[-4000:]}"
    with open(rp, "rb") as f:
        return f.read()


def result_bytes(o) -> bytes:
    return b"".join(np.ascontiguousarray(o[k]).tobytes() for k in KEYS) + o["counts"].tobytes()
