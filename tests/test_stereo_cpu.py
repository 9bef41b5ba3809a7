"""Stereo matching (slam_stereo_*) without a GPU: the host twin of csrc/stereo.hip (tests/stereo_twin.py: csrc/stereo_point.h, the
text the kernels run, built by g++) against the numpy statement on another route (tests/stereo_ref.py), hand cases whose answers
are written down from the specification, the sanitized stand-alone program, the extractor chain on the extractor's numpy
statement, the ABI table, every refusal that needs no device and the compiled kernels' metadata.  tests/test_stereo_gpu.py then
holds the device to the statement."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import stereo_cases as C
import stereo_ref as ref
import stereo_twin as tw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "slam-experiments_amd", "csrc")
NAMES = ("slam_stereo_workspace", "slam_stereo_match")
HAND = C.hand_cases()
RANDOM = ((1, [257, 65, 64], [257, 63, 1], 260), (2, [0, 1, 63], [64, 0, 65], 70), (3, [64, 257, 1], [0, 64, 257], 257))


def _pair_args(left, right, a, b):
    nL, nR = int(left["count"][a]), int(right["count"][b])
    return (left["kp"][a, :nL], left["desc"][a, :nL], left["planes"][a], right["kp"][b, :nR], right["desc"][b, :nR], right["planes"][b])


# ---- the twin against the statement -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,cl,cr,n_max", RANDOM)
def test_twin_equals_the_statement_on_random_blocks(seed, cl, cr, n_max):
    left, right = C.random_blocks(seed, cl, cr, n_max)
    for prm in (C.PARAMS3, dict(C.PARAMS3, reject=False, w=3, Ls=7, min_d=1.5, th_orb=60)):
        for b in range(len(cl)):
            args = _pair_args(left, right, b, b)
            want, got = ref.match_pair(*args, C.SCALE3, **prm), tw.match_pair(*args, C.SCALE3, **prm)
            assert tw.result_bytes(got) == tw.result_bytes(want), (seed, b)


def test_every_status_occurs_in_the_random_blocks():
    seed, cl, cr, n_max = RANDOM[0]
    left, right = C.random_blocks(seed, cl, cr, n_max)
    out = ref.match([(b, b) for b in range(len(cl))], left, right, C.SCALE3, **C.PARAMS3)
    assert (np.bincount(out["status"].ravel(), minlength=7) > 0).all()
    assert (out["status"][0, cl[0]:] == ref.NO_CANDIDATE).all() and np.isnan(out["depth"][0, cl[0]:]).all()


def test_sanitized_program_gives_the_twins_bytes():
    seed, cl, cr, n_max = RANDOM[0]
    left, right = C.random_blocks(seed, cl, cr, n_max)
    for b in (0, 2):
        args = _pair_args(left, right, b, b)
        assert tw.san_pair(*args, C.SCALE3, **C.PARAMS3) == tw.result_bytes(tw.match_pair(*args, C.SCALE3, **C.PARAMS3))
    empty = (np.zeros((0, 4), np.int32), np.zeros((0, 32), np.uint8), left["planes"][0])
    assert tw.san_pair(*empty, *empty, C.SCALE3, **C.PARAMS3) == np.zeros(2, np.int32).tobytes()
    for name, scene, prm, _ in HAND:
        assert tw.san_pair(*scene, **prm) == tw.result_bytes(tw.match_pair(*scene, **prm)), name


# ---- hand cases -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("impl", [ref, tw], ids=["statement", "twin"])
@pytest.mark.parametrize("case", HAND, ids=[c[0] for c in HAND])
def test_hand_cases(case, impl):
    name, scene, prm, expect = case
    C.check_expect(impl.match_pair(*scene, **prm), expect, name)


def test_the_hand_cases_cover_the_list():
    names = {c[0] for c in HAND}
    for want in ("band_floor_and_ceil", "level_gate_in", "level_gate_out", "disparity_low_bound_in", "disparity_high_bound_in", "left_of_min_d",
                 "duplicate_descriptors", "flat_patch", "symmetric_profile", "best_at_minus_Ls", "best_at_plus_Ls", "equal_sad_lower_inc_wins",
                 "window_left_minus_one", "window_left_zero", "window_right_level_w", "window_right_level_w_minus_one",
                 "disparity_zero_becomes_0_01", "median_n1_kept", "median_n2", "median_n3", "median_n4_equality_rejected", "median_off"):
        assert want in names, want


def test_parabola_alone():
    """den = 0 gives 0, not ORB-SLAM's NaN; |delta| <= 1/2 whenever d2 is the minimum.  (Through a pair den = 0 cannot occur: the
    lowest inc wins ties, so d1 > d2 at an interior best.  The flat patch is a slide border.)"""
    f = tw.lib().st_tw_parabola
    f.restype, f.argtypes = ctypes.c_double, [ctypes.c_int] * 3
    assert f(5, 5, 5) == 0.0 and f(0, 0, 0) == 0.0
    assert f(9, 1, 9) == 0.0 and f(9, 1, 1) == 0.5 and f(1, 1, 9) == -0.5
    rng = np.random.default_rng(5)
    for d1, d2, d3 in rng.integers(0, 61711, (200, 3)):
        d2 = min(d1, d2, d3)
        assert abs(f(int(d1), int(d2), int(d3))) <= 0.5
        den = d1 + d3 - 2 * d2
        assert f(int(d1), int(d2), int(d3)) == (0.0 if den == 0 else float(d1 - d3) / float(2 * den))


# ---- the extractor chain on the extractor's numpy statement ---------------------------------------------------------------------
@pytest.mark.parametrize("d", [3, 17])
def test_chain_truth_and_the_measured_counts_on_the_cpu(d):
    """n_levels = 1: the SAD at the true inc is 0 and |delta| <= 1/2, so every status-0 row whose best SAD is 0 lies within half
    a pixel of the true disparity (derived); their number is the one written in stereo_cases.py (measured)."""
    blk, sc = C.chain_cpu(d, 1)
    out = ref.match([(0, 1)], blk, blk, sc, bf=C.CHAIN_BF, max_d=C.CHAIN_MAX_D, reject=False)
    out["uL"] = ref.level0(blk["kp"][0, :, 0], sc[blk["kp"][0, :, 2]])
    n, err = C.chain_truth(out, d)
    print(f"d={d}: {n} status-0 rows with SAD 0, largest |disp - d| = {err:.4f}")
    assert err <= 0.5
    assert n == C.CHAIN_MEASURED[d] and C.CHAIN_FLOOR[d] == n // 2 and n >= 100
    # with the rejection on the median is 0 and no row survives it
    rej = ref.match([(0, 1)], blk, blk, sc, bf=C.CHAIN_BF, max_d=C.CHAIN_MAX_D, reject=True)
    assert rej["counts"][0, 0] == 0 and rej["counts"][0, 1] == out["counts"][0, 1]
    twin = tw.match_pair(*_pair_args(blk, blk, 0, 1), sc, bf=C.CHAIN_BF, max_d=C.CHAIN_MAX_D, reject=False)
    n0 = int(blk["count"][0])
    assert all(np.array_equal(twin[k], out[k][0, :n0], equal_nan=True) for k in ref.KEYS)


# ---- ABI, header, refusals ------------------------------------------------------------------------------------------------------
def test_header_abi_table_kernel_file_and_makefile_name_the_same_entry_points(built):
    from slamhip import _lib, stereo

    header = open(os.path.join(ROOT, "include", "slamhip.h")).read()
    lib = _lib.load()
    src = open(os.path.join(CSRC, "stereo.hip")).read()
    for name in NAMES:
        decl = re.search(r"SLAM_API int %s\((.*?)\);" % name, header, re.S).group(1)
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is ctypes.c_int and len(argtypes) == decl.count(",") + 1, name
        assert getattr(lib, name).argtypes == argtypes
        assert re.search(r'extern "C" int %s\(' % name, src)
    assert sorted(n for n in _lib.SIGNATURES if n.startswith("slam_stereo_")) == sorted(NAMES)
    assert sorted(set(re.findall(r'extern "C" int (slam_\w+)\(', src))) == sorted(NAMES)
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "stereo.hip" in mk and "stereo_point.h" in mk
    point = open(os.path.join(CSRC, "stereo_point.h")).read()
    assert point.index("#pragma clang fp contract(off)") < point.index("#include")
    for name, value, py in (("SLAM_STEREO_MAX_PAIRS", 4096, stereo.MAX_PAIRS), ("SLAM_STEREO_MAX_ROWS", 8192, stereo.MAX_ROWS),
                            ("SLAM_STEREO_MAX_LEVELS", 16, stereo.MAX_LEVELS), ("SLAM_STEREO_MAX_SIDE", 8192, stereo.MAX_SIDE),
                            ("SLAM_STEREO_HALF_MAX", 15, stereo.HALF_MAX)):
        assert re.search(r"#define %s %d\b" % (name, value), header) and py == value, name
    assert re.search(r"#define ST_HALF_MAX 15\b", point)
    assert (stereo.MATCHED, stereo.NO_CANDIDATE, stereo.ORB_DISTANCE, stereo.WINDOW, stereo.SLIDE_BORDER, stereo.DISPARITY, stereo.MEDIAN) == \
        (ref.MATCHED, ref.NO_CANDIDATE, ref.ORB_DISTANCE, ref.WINDOW, ref.SLIDE_BORDER, ref.DISPARITY, ref.MEDIAN)
    for k, name in enumerate(("ST_MATCHED", "ST_NO_CANDIDATE", "ST_ORB_DISTANCE", "ST_WINDOW", "ST_SLIDE_BORDER", "ST_DISPARITY", "ST_MEDIAN")):
        assert re.search(r"#define %s %d\b" % (name, k), point), name
    assert np.array_equal(stereo.scale_table(1.2, 8), np.float32(1.2) ** np.arange(8, dtype=np.float32))


def test_c_entry_points_refuse_bad_arguments_without_a_device(built):
    from slamhip import _lib

    lib = _lib.load()
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    one = ctypes.c_void_p(256)                        # a non-null, aligned "device" pointer: every call below is refused before it is read
    pairs = np.asarray([[0, 1]], np.int32)
    off = np.asarray([0, 4096], np.uint64)
    pitch, lw, lh = np.asarray([64, 56], np.int32), np.asarray([60, 50], np.int32), np.asarray([40, 33], np.int32)
    sc = ref.scale_table(1.2, 2)

    def run(ctx=one, Pn=1, pairs=pairs, BL=2, BR=2, blk=(one, one, one, one), blkR=None, n_max=100, L=2, off=off, pitch=pitch, lw=lw, lh=lh, sc=sc,
            bf=40.0, min_d=0.0, max_d=50.0, th=75, w=5, Ls=5, ws=one, ws_bytes=1 << 20, outs=(one,) * 7):
        blkR = blk if blkR is None else blkR
        q = lambda a: P(a) if a is not None else None  # noqa: E731
        return lib.slam_stereo_match(ctx, Pn, q(pairs), BL, *blk, BR, *blkR, n_max, L, 0, 8192, q(off), q(pitch), q(lw), q(lh), q(sc), bf, min_d,
                                     max_d, th, w, Ls, 1, ws, ws_bytes, *outs)

    def bad(rc, text):
        assert rc == _lib.SLAM_ERR_INVALID and text.encode() in lib.slam_last_error(), (rc, lib.slam_last_error())

    bad(run(ctx=None), "null ctx")
    bad(run(Pn=-1), "P=")
    bad(run(Pn=4097), "P=")
    bad(run(n_max=-1), "n_max=")
    bad(run(n_max=8193), "n_max=")
    bad(run(L=0), "L=")
    bad(run(L=17), "L=")
    bad(run(pairs=None), "h_pairs")
    bad(run(pairs=np.asarray([[2, 0]], np.int32)), "outside its blocks")
    bad(run(pairs=np.asarray([[0, 2]], np.int32)), "outside its blocks")
    bad(run(pairs=np.asarray([[-1, 0]], np.int32)), "outside its blocks")
    bad(run(BL=0), "outside its blocks")
    bad(run(th=-1), "th_orb")
    bad(run(th=257), "th_orb")
    for k in ("w", "Ls"):
        bad(run(**{k: 0}), "w=")
        bad(run(**{k: 16}), "w=")
    for v in (0.0, -1.0, np.inf, np.nan):
        bad(run(bf=v), "bf must be")
    for v in (np.inf, -np.inf, np.nan):
        bad(run(min_d=v), "min_d must be finite")
    bad(run(max_d=0.0), "max_d must be above")
    bad(run(min_d=3.0, max_d=3.0), "max_d must be above")
    bad(run(max_d=np.nan), "max_d must be above")
    for k in ("off", "pitch", "lw", "lh", "sc"):
        bad(run(**{k: None}), "null host pointer")
    bad(run(lw=np.asarray([0, 50], np.int32)), "level 0")
    bad(run(lh=np.asarray([40, 8193], np.int32)), "level 1")
    bad(run(pitch=np.asarray([59, 56], np.int32)), "pitch of level 0")
    bad(run(sc=np.asarray([1.0, 0.5], np.float32)), "h_scale[1]")
    bad(run(sc=np.asarray([np.nan, 1.2], np.float32)), "h_scale[0]")
    bad(run(ws=None), "workspace")
    bad(run(ws=ctypes.c_void_p(264)), "workspace")
    need = ctypes.c_uint64(0)
    assert lib.slam_stereo_workspace(1, 100, ctypes.byref(need)) == 0 and need.value >= 512 + 8
    bad(run(ws_bytes=need.value - 1), "workspace")
    for k in range(4):
        blk = [one] * 4
        blk[k] = None
        bad(run(blk=tuple(blk), blkR=(one,) * 4), "null device pointer (a block)")
        bad(run(blkR=tuple(blk)), "null device pointer (a block)")
    bad(run(blk=(one, ctypes.c_void_p(264), one, one)), "aligned to 16")
    bad(run(blk=(one, one, ctypes.c_void_p(260), one)), "aligned to 16")
    for k in range(7):
        outs = [one] * 7
        outs[k] = None
        bad(run(outs=tuple(outs)), "null device pointer (an output)")
    bad(run(outs=(one, ctypes.c_void_p(260), one, one, one, one, one)), "misaligned")
    bad(run(outs=(ctypes.c_void_p(258), one, one, one, one, one, one)), "misaligned")
    # nothing to do needs no device and no device pointers
    none4 = (None,) * 4
    assert run(Pn=0, pairs=None, blk=none4, ws=None, ws_bytes=0, outs=(None,) * 7) == 0
    assert run(n_max=0, blk=none4, ws=None, ws_bytes=0, outs=(None,) * 7) == 0
    bad(lib.slam_stereo_workspace(1, 100, None), "null bytes")
    bad(lib.slam_stereo_workspace(4097, 100, ctypes.byref(need)), "bad sizes")
    bad(lib.slam_stereo_workspace(1, 8193, ctypes.byref(need)), "bad sizes")
    assert lib.slam_stereo_workspace(4096, 8192, ctypes.byref(need)) == 0 and need.value >= 512 + 8 * 4096


def test_python_layer_raises_value_errors_before_the_library_is_touched(built, monkeypatch):
    from slamhip import stereo

    def touched(*a, **k):
        raise AssertionError("the library was touched")

    monkeypatch.setattr(stereo, "default_context", touched)
    monkeypatch.setattr(stereo, "stereo_match_device", touched)
    kp, desc = [np.asarray([[20, 20, 0, 0]], np.int32)], [np.zeros((1, 32), np.uint8)]
    planes = [[np.zeros((40, 48), np.uint8)]]
    sc = stereo.scale_table(1.2, 1)
    good = dict(bf=40.0, max_d=30.0)

    def arr(kpL=kp, descL=desc, plL=planes, kpR=kp, descR=desc, plR=planes, scale=sc, pairs=None, **kw):
        return stereo.stereo_match_arrays(kpL, descL, plL, kpR, descR, plR, scale, pairs, **{**good, **kw})

    for kw in (dict(bf=0.0), dict(bf=np.inf), dict(bf="x"), dict(min_d=np.nan), dict(max_d=0.0), dict(max_d=None), dict(th_orb=257), dict(th_orb=7.5),
               dict(w=0), dict(w=16), dict(Ls=0), dict(Ls=True)):
        with pytest.raises(ValueError):
            arr(**kw)
    with pytest.raises(ValueError):
        arr(pairs=[[0, 1]])
    with pytest.raises(ValueError):
        arr(pairs=[[0.0, 0.0]])
    with pytest.raises(ValueError):
        arr(scale=np.asarray([0.5], np.float32))
    with pytest.raises(ValueError):
        arr(kpL=[np.asarray([[48, 20, 0, 0]], np.int32)])                    # outside its level
    with pytest.raises(ValueError):
        arr(kpL=[np.asarray([[20, 20, 1, 0]], np.int32)])                    # a level the pyramid lacks
    with pytest.raises(ValueError):
        arr(descL=[np.zeros((1, 31), np.uint8)])
    with pytest.raises(ValueError):
        arr(plR=[[np.zeros((40, 50), np.uint8)]])                            # another pyramid shape
    with pytest.raises(ValueError):
        arr(kpR=kp + kp, descR=desc + desc, plR=planes + planes)             # 1 image against 2, no pairs
    with pytest.raises(ValueError):
        stereo.stereo_match(object(), None, None, bf=40.0, fx=400.0)         # one extractor needs pairs
    # nothing to match needs no device
    res = arr(kpL=[np.zeros((0, 4), np.int32)], descL=[np.zeros((0, 32), np.uint8)], kpR=[np.zeros((0, 4), np.int32)], descR=[np.zeros((0, 32), np.uint8)])
    assert len(res) == 1 and res.status[0].shape == (0,) and res.counts.tolist() == [[0, 0]]


# ---- the compiled kernels -------------------------------------------------------------------------------------------------------
def test_hipcc_compiles_the_kernels_for_gfx950_without_scratch(tmp_path):
    hipcc, readelf = "/opt/rocm/bin/hipcc", "/opt/rocm/llvm/bin/llvm-readelf"
    if not (os.path.exists(hipcc) and os.path.exists(readelf)):
        pytest.skip("hipcc / llvm-readelf of the ROCm toolchain not found")
    obj = str(tmp_path / "stereo.co")
    subprocess.run([hipcc, "--offload-arch=gfx950", "--cuda-device-only", "--no-gpu-bundle-output", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-DSLAM_BUILD", "-c",
                    os.path.join(CSRC, "stereo.hip"), "-o", obj], check=True, capture_output=True)
    notes = subprocess.run([readelf, "--notes", obj], check=True, capture_output=True, text=True).stdout
    kernels = {}
    for blk in re.split(r"\n\s+- \.agpr_count", notes)[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        kernels[name] = {k: int(re.search(rf"\.{k}:\s+(\d+)", blk).group(1))
                         for k in ("private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count", "vgpr_count", "sgpr_count",
                                   "group_segment_fixed_size")}
    assert sorted(re.sub(r"^_Z\d+(\w+?_kernel).*", r"\1", n) for n in kernels) == ["stereo_median_kernel", "stereo_sad_kernel", "stereo_search_kernel"]
    for name, m in kernels.items():
        print(name, m)
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, name
        assert m["vgpr_count"] <= 128 and m["group_segment_fixed_size"] <= 16384, name
