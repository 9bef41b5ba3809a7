"""Time of the lens-distortion calls (slam_cam_*), from HIP events (slam_timer_start/stop) around calls on device-resident
arrays, after a warm launch; the median and the spread (min - max) of 7 rounds are reported.  Every host figure (the Python
call with its copies, the C++ twin, numpy) is the BEST of 3 runs by the host clock, not a median.

    python tools/camera_time.py [--rounds R] > profiles/camera_time.log

  * points     slam_cam_undistort_f64 on 1 x 2000 and 64 x 2000 keypoints of the EuRoC cam0 model (10 Newton steps, and 6, where
               the iteration is at its floor), resident arrays; beside it the Python call (upload, launch, three downloads) and
               one host core: the numpy statement (tests/camera_ref.py, OpenCV's fixed-point iteration run to the end and, as OpenCV runs it, for 5 steps) and the
               host build of csrc/cam_model.h (tests/camera_twin.py, plain C++ at -O2);
  * map        slam_cam_rectify_map of one 752 x 480 camera, beside the numpy statement;
  * remap      slam_cam_remap_u8 of 1 and 64 frames of 752 x 480 through that map, with and without the mask, with the bytes the
               call must move (the source once, the map once, image and mask written once) over the time, beside the HBM
               figures of the MI355X (8.0 TB/s specified, 6.29 TB/s measured by a float4 copy); beside it the numpy statement.
The values are a record, not a gate."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "slam-experiments_amd"), os.path.join(ROOT, "tests"), ROOT):
    sys.path.insert(0, p)

import slamhip  # noqa: E402
import camera_cases as C  # noqa: E402
import camera_ref as ref  # noqa: E402
import camera_twin as tw  # noqa: E402

HBM_SPEC, HBM_COPY = 8.0e12, 6.29e12
W, H = C.EUROC.size


def opt(name, default):
    if name in sys.argv:
        i = sys.argv.index(name)
        v = sys.argv[i + 1]
        del sys.argv[i:i + 2]
        return type(default)(v)
    return default


def spread(v):
    return f"{np.median(v) * 1e3:10.1f} us  [{min(v) * 1e3:9.1f} - {max(v) * 1e3:9.1f}]"


def host(fn, repeat=3):
    """Best of ``repeat`` runs by the host clock, in microseconds."""
    best = np.inf
    for _ in range(repeat):
        t = time.perf_counter()
        fn()
        best = min(best, time.perf_counter() - t)
    return best * 1e6


def main():
    rounds = opt("--rounds", 7)
    ctx = slamhip.default_context()
    lib, h = ctx.lib, ctx.handle
    rng = np.random.default_rng(752480)
    cam = slamhip.CameraModel(*C.EUROC.K, C.EUROC.model, C.EUROC.coeffs)
    rec = np.ascontiguousarray(cam.record)
    P = lambda a: a.ctypes.data_as(__import__("ctypes").c_void_p)  # noqa: E731

    def timed(fn):
        ctx.timer_start()
        fn()
        return ctx.timer_stop()

    def run(call):
        timed(call)
        return [timed(call) for _ in range(rounds)]

    print(slamhip.load().slam_version().decode())
    tw.lib()
    for B in (1, 64):
        n = B * 2000
        px = np.stack([rng.uniform(0, W, n), rng.uniform(0, H, n)], -1)
        off = np.arange(B + 1, dtype=np.int64) * 2000
        d_in, d_out, d_norm, d_st = ctx.upload(px), ctx.malloc(16 * n), ctx.malloc(16 * n), ctx.malloc(n)

        def call(steps=10):
            assert lib.slam_cam_undistort_f64(h, B, P(off), 1, P(rec), None, steps, d_in.ptr, d_out.ptr, d_norm.ptr, d_st.ptr) == 0

        v6 = run(lambda: call(6))
        assert not d_st.download(np.uint8, (n,)).any()
        v = run(call)
        assert not d_st.download(np.uint8, (n,)).any()
        slamhip.undistort_points(px, cam, off, ctx=ctx)
        t_py = host(lambda: slamhip.undistort_points(px, cam, off, ctx=ctx))
        t_tw = host(lambda: tw.undistort(rec, px))
        t_np = host(lambda: ref.undistort_fixed_point(C.EUROC, px))
        t_cv = host(lambda: ref.undistort_fixed_point(C.EUROC, px, 5))
        print(f"points B = {B:2d} x 2000: {spread(v)}  {np.median(v) * 1e6 / n:8.2f} ns / point | host clock, best of 3: Python call with its copies {t_py:9.1f} us | "
              f"one host core: C++ twin {t_tw:9.1f} us, numpy fixed point to the end {t_np:9.1f} us, numpy 5 steps {t_cv:9.1f} us")
        print(f"points B = {B:2d} x 2000, 6 steps: {spread(v6)}")
        for b in (d_in, d_out, d_norm, d_st):
            b.free()

    K = np.asarray(cam.K)
    d_map = ctx.malloc(8 * W * H)

    def make_map():
        assert lib.slam_cam_rectify_map(h, P(rec), None, P(K), W, H, d_map.ptr) == 0

    v = run(make_map)
    t_np = host(lambda: ref.rectify_map(C.EUROC, (W, H), cam.K))
    print(f"map    {W} x {H}:      {spread(v)}  {np.median(v) * 1e6 / (W * H):8.3f} ns / entry | one host core, best of 3: numpy {t_np:9.1f} us")
    host_map = d_map.download(np.int32, (H, W, 2))

    for B in (1, 64):
        frames = rng.integers(0, 256, (B, H, W), dtype=np.uint8)
        d_src, d_dst, d_mask = ctx.upload(frames), ctx.malloc(B * H * W), ctx.malloc(B * H * W)
        for with_mask in (True, False):
            def call():
                assert lib.slam_cam_remap_u8(h, d_src.ptr, B, H, W, W, H * W, d_map.ptr, H, W, 0, d_dst.ptr, W, H * W,
                                             d_mask.ptr if with_mask else None) == 0

            v = run(call)
            moved = B * H * W * (2 + int(with_mask)) + 8 * H * W
            rate = moved / (np.median(v) * 1e-3)
            print(f"remap  B = {B:2d} {'with mask' if with_mask else 'no mask  '}: {spread(v)}  {np.median(v) * 1e3 / B:8.2f} us / frame | {moved / 1e6:7.2f} MB needed, "
                  f"{rate / 1e9:7.1f} GB/s = {100 * rate / HBM_COPY:5.1f} % of the 6.29 TB/s a copy reaches ({100 * rate / HBM_SPEC:5.1f} % of 8.0 TB/s)")
        k = min(B, 4)
        t_np = host(lambda: ref.remap(frames[:k], host_map, 0)) / k
        want = ref.remap(frames[:1], host_map, 0)
        assert np.array_equal(d_dst.download(np.uint8, (B, H, W))[:1], want[0])
        print(f"remap  B = {B:2d} one host core, best of 3: numpy {t_np:9.1f} us / frame")
        for b in (d_src, d_dst, d_mask):
            b.free()
    d_map.free()


if __name__ == "__main__":
    main()
