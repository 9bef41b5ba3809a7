"""Where a wave of a matrix-core top-2 search (bf_mx.hip, bf_mx32.hip) spends its life, by phase (development aid).

    python tools/mx_phase_probe.py LIB [NxM ...] [--warm K] [--engine 2|3] [--feed 0|1|2]

LIB is an experiment build of libslamhip.so with -DSLAM_MX_PROBE in the kernel's file (tools/build_variant.sh bf_mx
slam-experiments_amd/csrc/bf_mx.hip tools/exp/libslamhip_probe.so -mllvm -amdgpu-mfma-vgpr-form -DSLAM_MX_PROBE for the 16x16
kernel, engine 2, the default; the same with bf_mx32 twice for the 32x32 kernel, engine 3): every wave sums the shader clock
(s_memtime) over its phases and lane 0 leaves the sums in a buffer of this tool's at the end.  The shipped build executes no stamp.  The stamps cost time
(about one scalar memory instruction and a wait per phase boundary, two boundaries per stage more in a stage that fires): read
the SHARES, and the kernel time of the stamped build beside the shipped one's.

Per size, after K warm launches: the share of a wave's life in each phase, mean over all waves, and the same for wave 0 of
each block (the one that draws the tickets) and for waves 1-3."""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "slam-experiments_amd"))
from slamhip._lib import SIGNATURES  # noqa: E402

PHASES = ["prologue", "chunk start", "quiet scan", "update paths", "stage end", "stage barrier", "epilogue", "stage head"]



def opt(name, default):
    if name in sys.argv:
        i = sys.argv.index(name)
        v = int(sys.argv[i + 1])
        del sys.argv[i:i + 2]
        return v
    return default


warm, engine, feed = opt("--warm", 50), opt("--engine", 2), opt("--feed", 0)     # --feed: slam_bf_set_mx_feed (builds that have it)
assert engine in (2, 3), "--engine 2 (bf_top2_mx_kernel) or 3 (bf_top2_mx32_kernel)"
path = sys.argv[1]
sizes = [tuple(int(v) for v in a.split("x")) for a in sys.argv[2:]] or [(65536, 65536)]

lib = ctypes.CDLL(os.path.abspath(path), mode=os.RTLD_LOCAL | os.RTLD_NOW)
for name, (res, args) in SIGNATURES.items():
    fn = getattr(lib, name, None)
    if fn is not None:
        fn.restype, fn.argtypes = res, args
set_probe = lib.slam_exp_set_mx32_probe if engine == 3 else lib.slam_exp_set_mx_probe     # each kernel's file has its own buffer
set_probe.argtypes = [ctypes.c_void_p]
ctx = ctypes.c_void_p()
assert lib.slam_ctx_create(0, ctypes.byref(ctx)) == 0
assert lib.slam_bf_set_engine(ctx, engine) == 0
if feed:
    assert lib.slam_bf_set_mx_feed(ctx, feed) == 0


def malloc(nbytes):
    p = ctypes.c_void_p()
    assert lib.slam_malloc(ctx, nbytes, ctypes.byref(p)) == 0
    return p


def upload(a):
    a = np.ascontiguousarray(a)
    p = malloc(a.nbytes)
    assert lib.slam_upload(ctx, p, a.ctypes.data, a.nbytes) == 0
    return p


for n, m in sizes:
    q = np.random.default_rng(228).integers(0, 256, (n, 32), dtype=np.uint8)
    t = np.random.default_rng(229).integers(0, 256, (m, 32), dtype=np.uint8)
    dq, dt, di, dd = upload(q), upload(t), malloc(n * 8), malloc(n * 8)
    blocks = ((n + 255) // 256) * 256                    # at most 256 workers per query block
    nbytes = blocks * 4 * 8 * 8
    buf = upload(np.zeros(nbytes, np.uint8))
    for _ in range(warm):
        assert lib.slam_bf_knn2_u256(ctx, dq, n, dt, m, 0, di, dd) == 0
    lib.slam_sync(ctx)
    ms = ctypes.c_float(0)
    lib.slam_timer_start(ctx)
    for _ in range(20):
        lib.slam_bf_knn2_u256(ctx, dq, n, dt, m, 0, di, dd)
    lib.slam_timer_stop(ctx, ctypes.byref(ms))
    assert set_probe(buf) == 0
    assert lib.slam_bf_knn2_u256(ctx, dq, n, dt, m, 0, di, dd) == 0
    lib.slam_sync(ctx)
    assert set_probe(None) == 0
    out = np.empty(nbytes // 8, np.uint64)
    assert lib.slam_download(ctx, out.ctypes.data, buf, nbytes) == 0
    s = out.reshape(-1, 4, 8).astype(np.float64)
    s = s[s.sum(axis=(1, 2)) > 0]                        # the blocks of the launch
    life = s.sum(axis=2, keepdims=True)
    print(f"{n}x{m} engine {engine}: {len(s)} blocks, stamped build {ms.value / 20 * 1e3:.1f} us per launch; a wave's life: median {np.median(life):.0f} cycles "
          f"(p5 {np.percentile(life, 5):.0f}, p95 {np.percentile(life, 95):.0f})")
    share = s / life
    for i in (0, 1, 7, 2, 3, 4, 5, 6):
        print(f"  {PHASES[i]:>14}: {100 * share[:, :, i].mean():6.2f} % of a wave's life   (wave 0: {100 * share[:, 0, i].mean():6.2f} %, waves 1-3: "
              f"{100 * share[:, 1:, i].mean():6.2f} %; mean {s[:, :, i].mean():9.0f} cycles)")
    for p in (dq, dt, di, dd, buf):
        lib.slam_free(ctx, p)
