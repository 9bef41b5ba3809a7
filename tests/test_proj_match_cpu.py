"""The projection search without a device: the numpy reference against answers known by construction (depths
that are powers of two, scale 2.0, prefix descriptors), the predicted level against the logarithm it replaces, the host twin of
the per-point header under AddressSanitizer and UndefinedBehaviorSanitizer bit for bit, the new ABI entries and the argument
checks of the Python layer that are raised before a context exists."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import proj_match_cases as C
import proj_match_ref as R
from hamming_families import prefix_rows

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
I34 = np.eye(4)[:3]
S2, S2SQ = R.scale_tables(4, 2.0)


@pytest.fixture(scope="module")
def pm(built):
    from slamhip import proj_match as module
    return module


# ---- the reference against known answers -----------------------------------------------------------------------------------

def test_scale_tables_are_the_running_product():
    s, s2 = R.scale_tables(4, 2.0)
    assert s.tolist() == [1.0, 2.0, 4.0, 8.0] and s2.tolist() == [1.0, 4.0, 16.0, 64.0]
    s, s2 = R.scale_tables(8, 1.2)
    assert s[0] == 1.0 and s[1] == 1.2 and s[2] == 1.2 * 1.2 and s[3] == 1.2 * 1.2 * 1.2 and np.array_equal(s2, s * s)


def test_reference_gates_on_the_edge_points():
    xyz, rng, nrm, status, lp = C.edge_points()
    got = R.gates(xyz, I34, np.zeros(3), 2.0, C.CAMERA, C.BOUNDS, S2, S2SQ, rng, nrm)
    assert got[0].tolist() == status.tolist()
    assert got[3].tolist() == lp.tolist()
    assert np.isnan(got[1][status == 1]).all() and np.isnan(got[2][status == 1]).all()
    # exact pixels: u = 256 X / Z + 320
    assert got[1][0] == 320.0 and got[2][0] == 240.0
    k = int(np.flatnonzero((xyz[:, 0] == -2.5))[0])
    assert got[1][k] == 0.0 and got[0][k] == 0
    k = int(np.flatnonzero((xyz[:, 0] == 2.5))[0])
    assert got[1][k] == 640.0 and got[0][k] == 2
    assert (got[4][status == 0] == 2.0 * S2[lp[status == 0]]).all()


def test_reference_gates_without_the_optional_fields():
    xyz = np.array([[0.0, 0.0, 4.0], [0.0, 0.0, 2.0 ** 600], [0.5, 0.25, 2.0]])
    st, u, v, lp, r = R.gates(xyz, I34, np.zeros(3), 3.0, C.CAMERA, C.BOUNDS, S2, S2SQ)
    assert st.tolist() == [0, 0, 0] and lp.tolist() == [0, 0, 0] and r.tolist() == [3.0, 3.0, 3.0]
    assert (u[2], v[2]) == (384.0, 272.0)
    st, u, v, lp, r = R.gates(xyz, I34, np.zeros(3), 3.0, C.CAMERA, C.BOUNDS, S2, S2SQ, level=[2, 9, -4])
    assert lp.tolist() == [2, 3, 0] and r.tolist() == [12.0, 24.0, 3.0]          # the level is clamped into the table


def test_predicted_level_is_the_clamped_logarithm():
    """lp = ceil(log(dmax / d) / log 1.2) clamped to [0, n_levels - 1], on a sweep that stays clear of the boundaries."""
    s, s2 = R.scale_tables(8, 1.2)
    ratios = []
    for k in range(-3, 12):
        for f in (0.15, 0.5, 0.85):
            ratios.append(1.2 ** (k + f))                    # dmax / d strictly between two powers of 1.2
    ratios = np.array(ratios)
    d = 3.7
    xyz = np.tile([0.0, 0.0, d], (len(ratios), 1))
    dmax = d * ratios
    rng = np.stack([np.zeros_like(dmax), dmax * dmax], 1)
    st, _, _, lp, _ = R.gates(xyz, I34, np.zeros(3), 1.0, C.CAMERA, C.BOUNDS, s, s2, rng)
    live = st == 0                                           # ratios below 1 put the point beyond dmax: status 3
    assert (st[ratios < 1] == 3).all() and live[ratios > 1].all()
    want = [min(max(math.ceil(math.log(q) / math.log(1.2)), 0), 7) for q in ratios[live]]
    assert lp[live].tolist() == want


def tiny_frame():
    """Five frame rows about the pixel (320, 240) with prefix descriptors: every distance is a difference of prefix lengths."""
    xy = np.array([[320.0, 240.0], [323.0, 240.0], [320.0, 244.0], [330.0, 240.0], [316.5, 236.5]], np.float32)
    return dict(desc=prefix_rows([100, 104, 90, 100, 131]), xy=xy, level=np.array([0, 0, 1, 0, 0], np.int32))


def test_reference_window_is_strict_and_ordered():
    fr = tiny_frame()
    pts = dict(xyz=np.array([[0.0, 0.0, 4.0]]), desc=prefix_rows([101]))
    s1 = R.scale_tables(1, 1.0)
    # r = 4: rows 0 (d 1), 1 (d 3), 4 (d 30; 3.5 px off) are inside; row 2 sits at exactly v + r and is out; row 3 is far
    m12, cnt, t = R.search(pts, fr, I34, np.zeros(3), 4.0, C.CAMERA, C.BOUNDS, *s1)
    assert t["idx"].tolist() == [[0, 1]] and t["dist"].tolist() == [[1, 3]]
    # the ratio rule: both neighbours on level 0, 1 > 0.9 * 3 is false -> kept
    assert m12.tolist() == [0] and cnt == 1
    m12, _, t = R.search(pts, fr, I34, np.zeros(3), np.nextafter(4.0, 5.0), C.CAMERA, C.BOUNDS, *s1)
    assert t["idx"].tolist() == [[0, 1]]                                        # row 2 (d 11) is inside now but third
    m12, _, _ = R.search(pts, fr, I34, np.zeros(3), 4.0, C.CAMERA, C.BOUNDS, *s1, ratio=0.3)
    assert m12.tolist() == [-1]                                                  # 1 > 0.3 * 3: a same-level second neighbour rejects
    fr["level"] = np.array([0, 1, 1, 0, 0], np.int32)
    m12, _, _ = R.search(pts, fr, I34, np.zeros(3), 4.0, C.CAMERA, C.BOUNDS, *s1, ratio=0.3)
    assert m12.tolist() == [0]                                                   # ... on another level it does not
    m12, _, t = R.search(pts, fr, I34, np.zeros(3), 1.0, C.CAMERA, C.BOUNDS, *s1, ratio=0.0)
    assert t["idx"].tolist() == [[0, -1]] and m12.tolist() == [0]                # a missing second neighbour passes
    m12, _, _ = R.search(pts, fr, I34, np.zeros(3), 1.0, C.CAMERA, C.BOUNDS, *s1, th_high=1)
    assert m12.tolist() == [0]                                                   # d0 == th_high is kept
    m12, _, _ = R.search(pts, fr, I34, np.zeros(3), 1.0, C.CAMERA, C.BOUNDS, *s1, th_high=0)
    assert m12.tolist() == [-1]
    fr["taken"] = np.array([1, 0, 0, 0, 0], np.uint8)
    _, _, t = R.search(pts, fr, I34, np.zeros(3), 4.0, C.CAMERA, C.BOUNDS, *s1)
    assert t["idx"].tolist() == [[1, 4]] and t["dist"].tolist() == [[3, 30]]


def test_reference_level_rule_and_one_to_one():
    # identical descriptors on levels lp - 2 .. lp + 1 around a point with lp = 2 (d2 = 16, dmax2 = 256, scale 2)
    xy = np.tile(np.array([[320.0, 240.0]], np.float32), (4, 1))
    fr = dict(desc=prefix_rows([50, 50, 50, 50]), xy=xy, level=np.array([0, 1, 2, 3], np.int32))
    pts = dict(xyz=np.array([[0.0, 0.0, 4.0]]), desc=prefix_rows([50]), range=np.array([[1.0, 256.0]]))
    _, _, t = R.search(pts, fr, I34, np.zeros(3), 1.0, C.CAMERA, C.BOUNDS, S2, S2SQ)
    assert t["lp"].tolist() == [2] and t["idx"].tolist() == [[1, 2]]             # ranges: levels lp - 1 .. lp
    pts = dict(xyz=pts["xyz"], desc=pts["desc"], level=np.array([2], np.int32))
    _, _, t = R.search(pts, fr, I34, np.zeros(3), 1.0, C.CAMERA, C.BOUNDS, S2, S2SQ)
    assert t["idx"].tolist() == [[1, 2]]                                         # levels lp - 1 .. lp + 1, the first two by row
    _, _, t = R.search(pts, fr, I34, np.zeros(3), 1.0, C.CAMERA, C.BOUNDS, S2, S2SQ, offsets=(1, 1))
    assert t["idx"].tolist() == [[3, -1]]
    # two points on one row with equal distance: the lower point keeps it, the other is dropped
    fr = dict(desc=prefix_rows([50, 90]), xy=np.array([[320.0, 240.0], [321.0, 240.0]], np.float32), level=np.zeros(2, np.int32))
    pts = dict(xyz=np.array([[0.0, 0.0, 4.0], [0.0, 0.0, 8.0], [0.0, 0.0, 2.0]]), desc=prefix_rows([53, 47, 52]))
    m12, cnt, t = R.search(pts, fr, I34, np.zeros(3), 2.0, C.CAMERA, C.BOUNDS, *R.scale_tables(1, 1.0), ratio=10.0)
    assert t["dist"][:, 0].tolist() == [3, 3, 2] and m12.tolist() == [-1, -1, 0] and cnt == 1
    m12, _, _ = R.search(dict(xyz=pts["xyz"][:2], desc=pts["desc"][:2]), fr, I34, np.zeros(3), 2.0, C.CAMERA, C.BOUNDS,
                         *R.scale_tables(1, 1.0), ratio=10.0)
    assert m12.tolist() == [0, -1]


def test_reference_mutual_agreement():
    i, k = R.mutual(np.array([5, -1, 7, 2]), np.array([10, 11, 12, 13]), np.array([12, 10, 99]), np.array([7, 5, 2]))
    # point 0 -> row 5 = point 1 of side 2, whose match is row 10 = rows1[0]: agreed; point 2 -> row 7 = point 0 -> 12 = rows1[2]: agreed
    assert i.tolist() == [0, 2] and k.tolist() == [1, 0]
    S = np.c_[2.0 * np.eye(3), [1.0, 2.0, 3.0]]
    assert np.allclose(R.compose(S, R.invert(S)), I34) and np.allclose(R.compose(R.invert(S), S), I34)


# ---- the host twin of the per-point header ------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("proj_twin") / "proj_match_twin")
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "slam-experiments_amd", "csrc"),
                           os.path.join(HERE, "proj_match_twin.cpp"), "-o", out])

    def run(job: bytes, n: int):
        path = out + ".job"
        with open(path, "wb") as f:
            f.write(job)
        r = subprocess.run([out, path], capture_output=True, text=True)
        assert r.returncode == 0, f"sanitized twin failed ({r.returncode}):\n{r.stderr[-4000:]}"
        return C.parse_twin(r.stdout, n) if n else ()
    return run


def _same_gates(got, want):
    return all(C.same_bits(g, w) for g, w in zip(got, want[:4]))


def test_twin_equals_the_reference_on_the_edge_points(twin):
    xyz, rng, nrm, status, lp = C.edge_points()
    got = twin(C.twin_job(xyz, I34, np.zeros(3), 2.0, C.CAMERA, C.BOUNDS, S2, S2SQ, rng, nrm), len(xyz))
    want = R.gates(xyz, I34, np.zeros(3), 2.0, C.CAMERA, C.BOUNDS, S2, S2SQ, rng, nrm)
    assert got[0].tolist() == status.tolist() and got[3].tolist() == lp.tolist()
    assert _same_gates(got, want)


@pytest.mark.parametrize("fields", [(), ("range",), ("normal",), ("level",), ("range", "normal", "level")])
def test_twin_equals_the_reference_on_a_scene(twin, fields):
    pts, _, pose, _ = C.make_scene(7, 300)
    rng = np.random.default_rng(3)
    pts["xyz"][::17] *= -1.0                                  # some behind, some out of bounds
    A = pose + rng.normal(0, 0.01, (3, 4))
    Ow = rng.normal(0, 0.3, 3)
    s, s2 = R.scale_tables(8, 1.2)
    kw = {k: pts[k] for k in fields}
    kw["rng"] = kw.pop("range", None)
    got = twin(C.twin_job(pts["xyz"], A, Ow, 7.0, C.CAMERA, C.BOUNDS, s, s2, **kw), 300)
    want = R.gates(pts["xyz"], A, Ow, 7.0, C.CAMERA, C.BOUNDS, s, s2, **kw)
    assert len(set(want[0].tolist())) >= 2
    assert _same_gates(got, want)


# ---- ABI, limits, argument checks -----------------------------------------------------------------------------------------

def test_abi_has_the_projection_entries(pm):
    from slamhip import _lib
    names = ["slam_proj_match_limits", "slam_proj_match_plan_describe", "slam_proj_match_grid", "slam_proj_match_project",
             "slam_proj_match_search"]
    lib = _lib.load()
    for n in names:
        assert n in _lib.SIGNATURES and hasattr(lib, n)
    header = open(os.path.join(ROOT, "include", "slamhip.h")).read()
    for n in names:
        assert f"SLAM_API int {n}(" in header
    assert "ORBmatcher::SearchByProjection" in header and "Frame::isInFrustum" in header and "AssignFeaturesToGrid" in header
    assert ctypes.sizeof(_lib.ProjFrames) == 88 and ctypes.sizeof(_lib.ProjPoints) == 64 and ctypes.sizeof(_lib.ProjParams) == 120


def test_limits_and_plan(pm):
    from slamhip import bow, bow_match
    lim = pm.limits()
    assert lim["rows_per_image"] == pm.ROWS_MAX == bow.IMAGE_MAX == bow_match.ROWS_MAX == 8192
    assert lim["pairs_per_call"] == pm.PAIRS_MAX == 4096 and lim["levels"] == 16 and lim["scan_lanes"] == 64 and lim["pair_bytes"] == 176
    plan = pm.plan_describe(256, 256, 2000)
    assert plan["scan_blocks"] == 256 * 32 and plan["finish_blocks"] == 256 and plan["sort_blocks"] == 256
    assert plan["workspace_bytes"] >= 256 * 176 + 2 * 8 * 256 * 2000 + 4 * 256 * 2000
    from slamhip._lib import SlamHipError
    for args in ((1, 4097, 10), (1, 1, 8193), (-1, 1, 1)):
        with pytest.raises(SlamHipError):
            pm.plan_describe(*args)
    assert pm.match_index_pairs is bow_match.match_index_pairs


def test_c_entry_points_reject_bad_arguments_without_a_context(pm):
    from slamhip import _lib
    lib = _lib.load()
    assert lib.slam_proj_match_limits(None) == _lib.SLAM_ERR_INVALID
    off = np.array([0, 4], np.int64)
    assert lib.slam_proj_match_grid(None, *[None] * 4, _lib.addr(off), 1, 640, 480, 16, *[None] * 7) == _lib.SLAM_ERR_INVALID
    assert lib.slam_proj_match_search(*[None] * 7, 0, *[None] * 9) == _lib.SLAM_ERR_INVALID
    assert lib.slam_proj_match_project(*[None] * 6, 0, *[None] * 5) == _lib.SLAM_ERR_INVALID


def test_python_argument_checks(pm):
    with pytest.raises(ValueError):
        pm.scale_tables(0, 1.2)
    with pytest.raises(ValueError):
        pm.scale_tables(17, 1.2)
    s, s2 = pm.scale_tables(8, 1.2)
    assert np.array_equal(s, R.scale_tables(8, 1.2)[0]) and np.array_equal(s2, R.scale_tables(8, 1.2)[1])
    d = np.zeros((3, 32), np.uint8)
    xy = np.zeros((3, 2), np.float32)
    for kw in (dict(size=(0, 480)), dict(size=(640, 480), cell=0), dict(size=(640, 480), cell=1.5), dict(size=(640, 480), offsets=[0, 2]),
               dict(size=(640, 480), bins=[0, 1, 32]), dict(size=(640, 480), taken=[0, 1])):
        with pytest.raises(ValueError):
            pm.FrameGrids.from_arrays(d, xy, [0, 1, 2], **kw)
    with pytest.raises(ValueError):
        pm.FrameGrids.from_arrays(d, xy, [0, 1, 16], size=(640, 480))
    with pytest.raises(ValueError):
        pm.FrameGrids.from_arrays(np.zeros((8193, 32), np.uint8), np.zeros((8193, 2), np.float32), np.zeros(8193, np.int32), size=(640, 480))
    x = np.zeros((3, 3))
    for kw in (dict(dmin2=np.ones(3)), dict(normal=np.zeros((3, 2))), dict(level=[0, 1, 16]), dict(bins=[0, 1, -1]), dict(offsets=[0, 1])):
        with pytest.raises(ValueError):
            pm.PointSets(x, d, **kw)
    with pytest.raises(ValueError):
        pm.PointSets(np.zeros((2, 3)), d)
    with pytest.raises(ValueError):
        pm.search_by_projection(None, None, [(0, 0)], np.eye(4)[None])
    with pytest.raises(ValueError):
        pm.project_points(None, [0], np.eye(4)[None])
    for bad in (dict(th_high=1.5), dict(ratio=float("nan")), dict(lo=1, hi=0), dict(scale=(np.ones(17), np.ones(17)))):
        kw = dict(camera=C.CAMERA, bounds=C.BOUNDS, scale=(s, s2), th_high=100, ratio=0.9, cos2_limit=0.25, level_rule=True, lo=-1, hi=0)
        kw.update(bad)
        with pytest.raises(ValueError):
            pm._params(**kw)
    with pytest.raises(ValueError):
        pm._th_arg([1.0, 0.0], 2)
    with pytest.raises(ValueError):
        pm._poses_arg(np.zeros((2, 3, 3)), 2)
    assert np.allclose(pm.camera_centres(np.c_[2.0 * np.eye(3), [2.0, 4.0, 6.0]][None]), [[-1.0, -2.0, -3.0]])
