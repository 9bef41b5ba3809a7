"""A/B of two choices inside slam_cam_remap_u8 on the experiment library of `tools/build_exp.sh camera-remap`
(tools/exp/libslamhip_camremap.so, which reads both from the environment at every call): the workgroup target that sets how
many images a lane walks with one read of its map entries, and byte taps against paired 16-bit taps.

    tools/build_exp.sh camera-remap && python tools/camera_remap_ab.py > profiles/camera_remap_ab.log

8 and 64 frames of 752 x 480 through the EuRoC cam0 map, image + mask.  The settings alternate inside every round (5 rounds of
10 calls each between HIP events, after one warm call per setting), so drift of the machine falls on all of them alike; both
variants are first checked against each other byte for byte.  The values are a record, not a gate."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "slam-experiments_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
from slamhip import _lib  # noqa: E402

_lib.LIB_PATH = os.path.join(ROOT, "tools", "exp", "libslamhip_camremap.so")
import slamhip  # noqa: E402
import camera_cases as C  # noqa: E402

W, H = C.EUROC.size
TARGETS = (1024, 2048, 4096, 8192, 16384, 1 << 20)


def setting(wg, paired):
    os.environ["SLAM_EXP_REMAP_WG"] = str(wg)
    if paired:
        os.environ["SLAM_EXP_REMAP_PAIRED"] = "1"
    else:
        os.environ.pop("SLAM_EXP_REMAP_PAIRED", None)


def main():
    ctx = slamhip.default_context()
    lib, h = ctx.lib, ctx.handle
    cam = slamhip.CameraModel(*C.EUROC.K, C.EUROC.model, C.EUROC.coeffs)
    m = slamhip.RectifyMap(cam, (W, H), ctx=ctx)
    rng = np.random.default_rng(1)
    print(slamhip.load().slam_version().decode(), "- experiment library", os.path.relpath(_lib.LIB_PATH, ROOT))
    for B in (8, 64):
        frames = rng.integers(0, 256, (B, H, W), dtype=np.uint8)
        d_src, d_dst, d_mask = ctx.upload(frames), ctx.malloc(B * H * W), ctx.malloc(B * H * W)

        def call():
            assert lib.slam_cam_remap_u8(h, d_src.ptr, B, H, W, W, H * W, m.buf.ptr, H, W, 0, d_dst.ptr, W, H * W, d_mask.ptr) == 0

        outs = []
        for paired in (False, True):
            setting(4096, paired)
            call()
            outs.append((d_dst.download(np.uint8, (B, H, W)), d_mask.download(np.uint8, (B, H, W))))
        assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
        settings = [(wg, False) for wg in TARGETS] + [(4096, True)]
        res = {s: [] for s in settings}
        for _ in range(5):
            for s in settings:
                setting(*s)
                call()
                ctx.timer_start()
                for _ in range(10):
                    call()
                res[s].append(ctx.timer_stop() / 10)
        for (wg, paired), v in res.items():
            print(f"B = {B:2d} target {wg:8d} {'paired 16-bit taps' if paired else 'byte taps         '}: median {np.median(v) * 1e3:8.1f} us  "
                  f"[{min(v) * 1e3:8.1f} - {max(v) * 1e3:8.1f}]", flush=True)
        for b in (d_src, d_dst, d_mask):
            b.free()
    m.free()


if __name__ == "__main__":
    main()
