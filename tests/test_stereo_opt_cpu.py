"""CPU: the statement of the stereo / level-weighted adjustments (tests/stereo_opt_ref.py) and the host twin of
csrc/stereo_edge.h - Jacobians against central differences in np.longdouble with a derived bar, the twin against the
statement bit for bit (also through the sanitized stand-alone program), the conditions the pose scenes must meet, the frame
on which only the stereo edges fix the translation norm, and the ABI table, header and refusals of the new entry points."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stereo_edge_twin as tw  # noqa: E402
import stereo_opt_cases as C  # noqa: E402
import stereo_opt_ref as S  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "slam-experiments_amd", "csrc")
NAMES = ("slam_reproj_rj_stereo_f64", "slam_pose_optimize_stereo_batch_f64", "slam_bas_linearize_stereo_f64", "slam_bas_cost_stereo_f64",
         "slam_bas_classify_stereo_f64")
LD = np.longdouble


def _table(seed=3, O=257, K=5, L=40):
    """A mixed observation table: both kinds, levels 0..7, s = 0 rows, a point at Z <= 0 (behind pose 1), a stereo edge at 0.5
    baselines and one at 400 baselines."""
    rng = np.random.default_rng(seed)
    T, X = C.R.scene(rng, K, L)
    T12 = T[:, :3, :4].reshape(K, 12)
    X[0] = -T[1, :3, :3].T @ T[1, :3, 3] - 2.0 * T[1, 2, :3]             # 2 m behind pose 1
    X[1] = -T[2, :3, :3].T @ T[2, :3, 3] + 0.5 * C.BASELINE * T[2, 2, :3]   # 0.5 baselines in front of pose 2
    X[2] = -T[3, :3, :3].T @ T[3, :3, 3] + 400 * C.BASELINE * T[3, 2, :3]   # 400 baselines in front of pose 3
    op, ol = rng.integers(0, K, O).astype(np.int32), rng.integers(3, L, O).astype(np.int32)
    op[:3], ol[:3] = [1, 2, 3], [0, 1, 2]
    pc = np.einsum("oij,oj->oi", T[op, :3, :3], X[ol]) + T[op, :3, 3]
    u = C.FX * pc[:, 0] / pc[:, 2] + C.CX
    meas3 = np.stack([u, C.FY * pc[:, 1] / pc[:, 2] + C.CY, u - C.BF / pc[:, 2]], 1) + rng.normal(0, 1.5, (O, 3))
    meas3[3::2, 2] = np.nan
    info = 1.0 / C.SCALE[np.arange(O) % 8] ** 2
    info[5::17] = 0.0
    return T12, X, op, ol, meas3, info


# ---- Jacobians -------------------------------------------------------------------------------------------------------------
def test_analytic_jacobians_against_central_differences_in_longdouble():
    """Every entry of Jp and Jq of the statement (run in np.longdouble) against central differences of its own residual, pose
    perturbed as T <- Exp(h e_a) T and point as p + h e_c.  The bar is derived, not picked: a central difference of step h has
    truncation h^2 / 6 |f'''| and rounding eps |f| / h; the residual is fx X / Z + .. with third derivatives of the order of
    M / zmin^3 (M the largest Jacobian entry's natural scale fx (1 + r^2), r the largest |X / Z|, |Y / Z|; lengths in metres,
    zmin the smallest depth, at least 1 for the pose directions since rotations move a point by its own length), so
    bar = 10 (h^2 M (1 + 1 / zmin^3) + eps_ld |e|max / h) per entry.  Includes a stereo edge at Z = 0.5 baselines and one at
    400 baselines; s = 0 rows and the row at Z <= 0 have Jacobians like any other."""
    T12, X, op, ol, meas3, info = _table()
    h = LD(1e-7)
    eps = np.finfo(LD).eps
    P, p = T12[op].astype(LD), X[ol].astype(LD)
    E = S.edge(P, p, meas3, info, C.CAM, dtype=LD)

    def resid(Pm, pm):
        return S.edge(Pm, pm, meas3, info, C.CAM, dtype=LD)["e"]

    def moved(a, sgn):
        xi = np.zeros(6, LD)
        xi[a] = sgn * h
        G = S._exp(xi, LD)
        Tm = np.concatenate([P.reshape(-1, 3, 4), np.broadcast_to(np.array([0, 0, 0, 1], LD), (len(P), 1, 4))], 1)
        return np.einsum("ij,ojk->oik", G, Tm)[:, :3, :].reshape(-1, 12)

    num_p = np.stack([(resid(moved(a, 1), p) - resid(moved(a, -1), p)) / (2 * h) for a in range(6)], 2)
    num_q = np.stack([(resid(P, p + h * np.eye(3, dtype=LD)[c]) - resid(P, p - h * np.eye(3, dtype=LD)[c])) / (2 * h) for c in range(3)], 2)
    Z = np.abs(E["Z"])
    r = np.maximum(np.abs(E["X"] / E["Z"]), np.abs(E["Y"] / E["Z"]))
    length = np.sqrt(E["X"] ** 2 + E["Y"] ** 2 + E["Z"] ** 2)
    M = (C.FX + C.BF / Z) * (1 + r * r)
    emax = np.abs(E["e"]).max(1) + C.FX * (1 + r)
    bar_q = 10 * (h * h * M * (1 + 1 / Z ** 3) + eps * emax / h)
    bar_p = 10 * (h * h * M * (1 + 1 / Z ** 3) * np.maximum(length, 1) ** 3 + eps * emax / h)
    worst_p = (np.abs(num_p - E["Jp"]) / bar_p[:, None, None]).max()
    worst_q = (np.abs(num_q - E["Jq"]) / bar_q[:, None, None]).max()
    print(f"\ncentral differences: worst |difference| / bar: pose {float(worst_p):.3g}, point {float(worst_q):.3g}; "
          f"largest bar {float(max(bar_p.max(), bar_q.max())):.3g}, smallest depth {float(Z.min()):.3g} m")
    assert worst_p <= 1 and worst_q <= 1
    assert E["stereo"][1] and E["stereo"][2] and abs(float(E["Z"][1]) / C.BASELINE - 0.5) < 1e-9 and abs(float(E["Z"][2]) / C.BASELINE - 400) < 1e-6
    assert float(E["Z"][0]) < 0
    # the analytic entries are not trivially small: the bar separates a wrong sign or a missing term
    assert float(np.abs(E["Jp"][E["stereo"], 2]).max() / bar_p.max()) > 1e6


def test_float64_statement_is_the_longdouble_one_rounded():
    T12, X, op, ol, meas3, info = _table()
    a = S.edge(T12[op], X[ol], meas3, info, C.CAM, S.DELTAS)
    b = S.edge(T12[op], X[ol], meas3, info, C.CAM, S.DELTAS, dtype=LD)
    ok = np.abs(a["Z"]) > 0.5                                # the 0.5-baseline edge divides by 0.055 m: its rounding is its own
    for k in ("e", "chi2", "Jp", "Jq"):
        d = np.abs(a[k][ok] - b[k][ok].astype(np.float64))
        assert (d <= 1e-9 * (1 + np.abs(a[k][ok]))).all(), k


# ---- the twin ---------------------------------------------------------------------------------------------------------------
def _same(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in tw.KEYS) and a["count"] == b["count"]


@pytest.mark.parametrize("deltas", [(0.0, 0.0), S.DELTAS, (1.0, 0.0)])
def test_twin_equals_the_statement_bit_for_bit(deltas):
    """stereo_edge.h built for the host against the numpy statement on the mixed table (s = 0, mr NaN, Z <= 0, both depth
    extremes), with a bad pose index, a bad point index, a negative and a NaN information: every output, the inlier flags and
    the count."""
    T12, X, op, ol, meas3, info = _table()
    op, ol, info = op.copy(), ol.copy(), info.copy()
    op[40], ol[41], info[42], info[43] = len(T12), -1, -1.0, np.nan
    got = tw.edges(T12, X, op, ol, meas3, info, C.CAM, deltas)
    ref = S.edges_table(T12, X, op, ol, meas3, info, C.CAM, deltas)
    assert _same(got, ref), [k for k in tw.KEYS if not np.array_equal(got[k], ref[k], equal_nan=True)]
    assert got["count"] == 4 and np.isnan(got["e"][40]).all() and np.isnan(got["Jpoint"][41]).all()
    assert got["chi2"][42] == 0 and got["chi2"][43] == 0 and not got["inlier"][[40, 41, 42, 43]].any()
    assert (got["e"][np.isnan(meas3[:, 2]) & (op < len(T12)) & (ol >= 0), 2] == 0).all()
    assert not got["inlier"][0] and got["chi2"][5] == 0 and not got["inlier"][5]        # Z <= 0; s = 0


@pytest.mark.parametrize("name", list(C.POSE_SCENES))
def test_twin_equals_the_statement_on_every_pose_scene(name):
    f = C.pose_scene(name)
    O = len(f["X"])
    T12 = f["T_init"][:3, :4].reshape(1, 12)
    got = tw.edges(T12, f["X"], np.zeros(O, np.int32), np.arange(O, dtype=np.int32), f["meas3"], f["info"], C.CAM, S.DELTAS)
    ref = S.edges_table(T12, f["X"], np.zeros(O, np.int32), np.arange(O), f["meas3"], f["info"], C.CAM, S.DELTAS)
    assert _same(got, ref)


def test_sanitized_program_returns_the_library_bytes():
    """The same source as a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer (nothing is preloaded):
    O = 0, the mixed table with its bad indices, and a scene beyond the stage."""
    T12, X, op, ol, meas3, info = _table()
    op = op.copy()
    op[40] = -7
    f = C.pose_scene("stage+1")
    O = len(f["X"])
    jobs = [(T12, X, op[:0], ol[:0], meas3[:0], info[:0]), (T12, X, op, ol, meas3, info),
            (f["T_init"][:3, :4].reshape(1, 12), f["X"], np.zeros(O, np.int32), np.arange(O, dtype=np.int32), f["meas3"], f["info"])]
    for job in jobs:
        assert tw.san_edges(*job, C.CAM, S.DELTAS) == tw.result_bytes(tw.edges(*job, C.CAM, S.DELTAS))


# ---- scene conditions ---------------------------------------------------------------------------------------------------------
_lm = {}


def _statement(name):
    if name not in _lm:
        f = C.pose_scene(name)
        _lm[name] = S.pose_lm(f["T_init"], f["X"], f["meas3"], f["info"], C.CAM)
    return _lm[name]


@pytest.mark.parametrize("name", list(C.POSE_SCENES))
def test_pose_scenes_meet_their_conditions(name):
    """On the statement alone: no edge's final weighted chi2 within 0.1 % of its gate (inlier sets are compared exactly), a
    monocular and a stereo edge rejected, an edge accepted on at least three pyramid levels, an edge with s = 0; the planted
    outliers are the rejected ones and the pose lands on the truth."""
    f = C.pose_scene(name)
    T, inl, chi2, acc, n_stereo = _statement(name)
    stereo = ~np.isnan(f["meas3"][:, 2])
    gate = np.where(stereo, S.CHI2_STEREO, S.CHI2_MONO)
    ratio = chi2 / gate
    assert not ((ratio >= 0.999) & (ratio <= 1.001)).any()
    on = f["info"] > 0
    assert (~inl & on & ~stereo).any() and (~inl & on & stereo).any()
    assert len(set(f["level"][inl].tolist())) >= 3
    assert (~on).any() and not inl[~on].any()
    assert not inl[f["bad"]].any() and inl[on & ~f["bad"]].mean() > 0.9
    assert n_stereo == int((inl & stereo).sum()) and acc >= 4
    d = T @ np.linalg.inv(f["T"])
    # a plausibility check of the scene, not of a kernel: nine good edges of up to 2 px noise at 6..15 m leave decimetres
    assert np.linalg.norm(d[:3, 3]) < (0.05 if len(inl) >= 100 else 0.2), np.linalg.norm(d[:3, 3])


# ---- what needs the feature ---------------------------------------------------------------------------------------------------
def test_only_the_stereo_edges_recover_the_translation_norm():
    """The frame of stereo_opt_cases.depth_shift_frame: the map lies 1.5 m deeper along every viewing ray, which monocular
    reprojection cannot see.  The statement's optimisation with u_right recovers |t| = 1.5 m; the same edges with every mr NaN
    stay where they started.  Bar: the depth noise of ONE stereo point of the scene, sigma_d Z^2 / bf = 0.3 * 8^2 / 50.45 =
    0.38 m (the estimate averages 160 of them, and carries the pull of the monocular rows, second order in the 0.005 cone).
    Recorded: stereo error 0.343 m, monocular error 1.457 m."""
    f = C.depth_shift_frame()
    bar = f["sigma_d"] * f["depth"] ** 2 / C.BF
    Ts, inl_s, *_ = S.pose_lm(f["T_init"], f["X"], f["meas3"], f["info"], C.CAM)
    mono3 = f["meas3"].copy()
    mono3[:, 2] = np.nan
    Tm, inl_m, *_ = S.pose_lm(f["T_init"], f["X"], mono3, f["info"], C.CAM)
    err_s = abs(np.linalg.norm(Ts[:3, 3]) - f["shift"])
    err_m = abs(np.linalg.norm(Tm[:3, 3]) - f["shift"])
    print(f"\ntranslation norm: stereo error {err_s:.3f} m, monocular error {err_m:.3f} m, bar {bar:.3f} m")
    assert 0.3 < bar < 0.45
    assert err_s <= bar < err_m
    assert inl_s.mean() > 0.9 and inl_m.mean() > 0.9


# ---- ABI, header, refusals ----------------------------------------------------------------------------------------------------
def test_header_abi_table_kernel_files_and_makefile_name_the_same_entry_points(built):
    from slamhip import _lib, stereo_opt

    header = open(os.path.join(ROOT, "include", "slamhip.h")).read()
    lib = _lib.load()
    src = open(os.path.join(CSRC, "ba_stereo.hip")).read() + open(os.path.join(CSRC, "pose_stereo.hip")).read()
    for name in NAMES:
        decl = re.search(r"SLAM_API int %s\((.*?)\);" % name, header, re.S).group(1)
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is ctypes.c_int and len(argtypes) == decl.count(",") + 1, name
        assert getattr(lib, name).argtypes == argtypes
        assert re.search(r'extern "C" int %s\(' % name, src)
    assert sorted(set(re.findall(r'extern "C" int (slam_\w+)\(', src))) == sorted(NAMES)
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert all(n in mk for n in ("ba_stereo.hip", "pose_stereo.hip", "stereo_edge.h", "pose_lm.h", "ba_sparse_common.h"))
    edge = open(os.path.join(CSRC, "stereo_edge.h")).read()
    code = "\n".join(line.split("//")[0] for line in edge.splitlines())
    assert "#pragma clang fp contract" not in code and "fma(" not in code
    for f in ("ba_stereo.hip", "pose_stereo.hip"):
        text = open(os.path.join(CSRC, f)).read()
        assert text.index("#pragma clang fp contract(off)") < text.index('#include "stereo_edge.h"')
        assert not re.search(r"\b(slam_workspace|slam_io_arena|radius_tables)\(ctx\b", text)
    assert f"#define SLAM_POSE_STEREO_STAGE {stereo_opt.STAGE}" in header and C.STAGE == stereo_opt.STAGE


def test_raw_entry_points_refuse_before_any_launch(built):
    """SLAM_ERR_INVALID without a context and, with the checks that come before the device is touched, for bf <= 0, negative
    gates and widths: none of these needs a GPU."""
    from slamhip import _lib

    lib = _lib.load()
    for name in NAMES:
        n = len(_lib.SIGNATURES[name][1])
        assert getattr(lib, name)(*([None] + [0] * (n - 1))) == _lib.SLAM_ERR_INVALID
        assert name.encode() in lib.slam_last_error()


def test_python_refuses_bad_arguments_before_any_allocation(built):
    import slamhip
    from slamhip import StereoEdges

    f = C.pose_scene("o12")
    ok = StereoEdges(f["meas3"], f["info"], C.BF)
    bad = [
        dict(bf=0.0), dict(bf=-1.0), dict(bf=np.nan), dict(gates=(-1.0, 7.8)), dict(gates=(5.9,)), dict(deltas=(-1.0, 1.0)), dict(rounds=-1),
        dict(iterations=1001), dict(edges=StereoEdges(f["meas3"][:-1], f["info"], C.BF)), dict(edges=StereoEdges(f["meas3"], f["info"][:-1], C.BF)),
        dict(edges=StereoEdges(f["meas3"], -f["info"], C.BF)), dict(edges=StereoEdges(f["meas3"], f["info"], 2 * C.BF)),
        dict(edges=StereoEdges(np.where(np.isnan(f["meas3"]), np.inf, f["meas3"]), f["info"], C.BF)),
    ]
    for kw in bad:
        kw = dict(kw)
        edges = kw.pop("edges", ok)
        bf = kw.pop("bf", C.BF)
        with pytest.raises(ValueError):
            slamhip.optimize_poses_stereo(f["T_init"][None], [f["X"]], [edges], C.R.INTR, bf, ctx=object(), **kw)
    with pytest.raises(ValueError):
        slamhip.optimize_poses_stereo(f["T_init"][None], [f["X"], f["X"]], [ok], C.R.INTR, C.BF, ctx=object())
    w = C.local_window()
    st = StereoEdges(w["meas3"], w["info"], C.BF)
    for kw in (dict(stereo=StereoEdges(w["meas3"][:-1], w["info"][:-1], C.BF)), dict(stereo=StereoEdges(w["meas3"], w["info"], 0.0)),
               dict(gates=(-1.0, 1.0)), dict(first=-1), dict(fixed_poses=())):
        args = dict(stereo=st, fixed_poses=w["fixed"])
        args.update(kw)
        with pytest.raises(ValueError):
            slamhip.local_bundle_adjust(w["T0"], w["X0"], w["op"], w["ol"], intrinsics=C.R.INTR, ctx=object(), **args)
    with pytest.raises(ValueError):
        slamhip.stereo_edge_linearization(w["T0"], w["X0"], w["op"], w["ol"][:-1], st, C.R.INTR, ctx=object())
    with pytest.raises(ValueError):
        slamhip.bundle_adjust_sparse(w["T0"], w["X0"], w["op"], w["ol"], None, C.R.INTR, fixed_poses=w["fixed"], huber_delta=(-1.0, 1.0),
                                     stereo=st, ctx=object())


def test_stereo_edges_from_a_stereo_result():
    """mu, mv from xy, mr = u_right where matched and NaN elsewhere, info = 1 / scale[level]^2, rows and refusals."""
    from slamhip import stereo_edges

    class Result:
        scale = np.float32(1.2) ** np.arange(4, dtype=np.float32)
        bf = 40.0
        status = [np.array([0, 3, 0, 6], np.uint8)]
        u_right = [np.array([100.25, np.nan, 7.5, np.nan])]
        xy = [np.array([[110.0, 50.0], [20.5, 30.0], [9.0, 8.0], [1.0, 2.0]], np.float32)]
        level = [np.array([0, 1, 3, 2], np.int32)]

        def __len__(self):
            return 1

    e = stereo_edges(Result(), 0)
    assert np.array_equal(e.meas3[:, :2], Result.xy[0].astype(np.float64)) and e.bf == 40.0
    assert np.array_equal(e.meas3[:, 2], [100.25, np.nan, 7.5, np.nan], equal_nan=True)
    s = Result.scale.astype(np.float64)
    assert np.array_equal(e.info, 1.0 / (s[[0, 1, 3, 2]] * s[[0, 1, 3, 2]]))
    sub = stereo_edges(Result(), 0, rows=[2, 0], scale=[1.0, 2.0, 4.0, 8.0])
    assert np.array_equal(sub.meas3[:, 2], [7.5, 100.25]) and np.array_equal(sub.info, [1 / 64.0, 1.0])
    for kw in (dict(b=1), dict(b=0, rows=[4]), dict(b=0, scale=[1.0, 1.2]), dict(b=0, scale=[1.0, 0.0, 1.0, 1.0])):
        with pytest.raises(ValueError):
            stereo_edges(Result(), **kw)
