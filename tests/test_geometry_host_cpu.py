"""The texts of the checks the four batched RANSAC estimators (two_view, pnp, homography, sim3) share, pinned: the size checks,
the null-pointer rule and the null-context rule of their C entry points as ``slam_last_error`` hands them to a caller, and the
``ValueError`` / ``TypeError`` texts of their Python wrappers and loop-edge builders.

Every check here is made in front of the first device call, so none of this needs a GPU: the C entry points get a handle that
is never dereferenced (a bad argument is found first)."""
import ctypes

import numpy as np
import pytest

K = np.array([[458.654, 0.0, 367.215], [0.0, 457.296, 248.375], [0.0, 0.0, 1.0]])
CAM = (458.654, 457.296, 367.215, 248.375)

_BUF = (ctypes.c_char * 1024)()
P = (ctypes.addressof(_BUF) + 15) // 16 * 16        # 16-byte aligned, as the two-view calls ask of their points


# name -> the arguments of a valid call in the order of the C signature, every pointer `p`
RANSAC = {
    "slam_tv_essential_ransac_f64": lambda p: dict(ctx=p, B=1, off=p, a=p, b=p, M=4, fx=CAM[0], fy=CAM[1], cx=CAM[2], cy=CAM[3], H=8, thr=1.0,
                                                   seed=0, model=p, inl=p, st=p),
    "slam_pnp_ransac_f64": lambda p: dict(ctx=p, B=1, off=p, a=p, b=p, M=4, fx=CAM[0], fy=CAM[1], cx=CAM[2], cy=CAM[3], H=8, thr=1.0, seed=0,
                                          model=p, inl=p, st=p),
    "slam_hg_ransac_f64": lambda p: dict(ctx=p, B=1, off=p, a=p, b=p, M=4, H=8, thr=1.0, seed=0, model=p, inl=p, st=p),
    "slam_sim3_ransac_f64": lambda p: dict(ctx=p, B=1, off=p, a=p, b=p, M=4, sg=None, fx=CAM[0], fy=CAM[1], cx=CAM[2], cy=CAM[3], H=8,
                                           gate=9.21, fix=0, seed=0, model=p, inl=p, st=p),
}
MINIMAL = {
    "slam_tv_fivepoint_f64": lambda p: dict(ctx=p, S=1, a=p, b=p, model=p, ok=p),
    "slam_pnp_p3p_f64": lambda p: dict(ctx=p, S=1, a=p, b=p, model=p, ok=p),
    "slam_hg_fourpoint_f64": lambda p: dict(ctx=p, S=1, a=p, b=p, model=p, ok=p),
    "slam_sim3_threepoint_f64": lambda p: dict(ctx=p, S=1, a=p, b=p, fix=0, model=p, ok=p),
}
# (arguments, cap of B, the pointers that may not be null)
PER_CANDIDATE = {
    "slam_tv_recover_pose_f64": (lambda p: dict(ctx=p, B=1, off=p, a=p, b=p, M=4, fx=CAM[0], fy=CAM[1], cx=CAM[2], cy=CAM[3], E=p, inl=None,
                                                dist=50.0, pose=p, good=p, st=p), 1 << 20, ("off", "a", "b", "E", "pose", "good", "st")),
    "slam_hg_decompose_f64": (lambda p: dict(ctx=p, B=1, off=p, a=p, b=p, M=4, fx=CAM[0], fy=CAM[1], cx=CAM[2], cy=CAM[3], Hm=p, inl=None,
                                             dist=50.0, pa=p, na=p, cnt=p, pose=p, sv=p, good=p, st=p), 1 << 20,
                              ("off", "a", "b", "Hm", "pa", "na", "cnt", "pose", "sv", "good", "st")),
    "slam_hg_model_score_f64": (lambda p: dict(ctx=p, B=1, off=p, a=p, b=p, M=4, fx=CAM[0], fy=CAM[1], cx=CAM[2], cy=CAM[3], Hm=p, E=p,
                                               sigma=1.0, score=p, ratio=p), 1 << 20, ("off", "a", "b", "Hm", "E", "score", "ratio")),
    "slam_sim3_refit_f64": (lambda p: dict(ctx=p, B=1, off=p, a=p, b=p, M=4, mask=None, fix=0, model=p, st=p), 1 << 24,
                            ("off", "a", "b", "model", "st")),
}


def _refused(lib, name, args, text):
    from slamhip import _lib

    assert getattr(lib, name)(*args.values()) == _lib.SLAM_ERR_INVALID, (name, args)
    assert lib.slam_last_error().decode() == text, (name, args)


@pytest.mark.parametrize("name", sorted(RANSAC))
def test_ransac_entry_point_texts(built, name):
    from slamhip import _lib

    lib, make = _lib.load(), RANSAC[name]
    _refused(lib, name, dict(make(P), ctx=None), f"{name}: null ctx")
    for kw in (dict(B=-1), dict(B=65536), dict(M=-1), dict(M=(1 << 28) + 1)):
        a = dict(make(P), **kw)
        _refused(lib, name, a, f"bad sizes (B={a['B']}, M={a['M']}; B <= 65535)")
    for H in (0, -3, (1 << 20) + 1):
        _refused(lib, name, dict(make(P), H=H), f"H={H} out of range [1, 2^20]")
    for field in ("off", "a", "b", "model", "inl", "st"):
        _refused(lib, name, dict(make(P), **{field: None}), f"{name}: null device pointer")
    a = dict(make(P), M=0, a=None, b=None, inl=None, off=None)       # with no correspondences only their three pointers may be null
    _refused(lib, name, a, f"{name}: null device pointer")
    assert getattr(lib, name)(*dict(make(P), B=0, off=None, model=None, st=None).values()) == _lib.SLAM_OK      # nothing to do, nothing read


@pytest.mark.parametrize("name", sorted(MINIMAL))
def test_minimal_solver_entry_point_texts(built, name):
    from slamhip import _lib

    lib, make = _lib.load(), MINIMAL[name]
    _refused(lib, name, dict(make(P), ctx=None), f"{name}: null ctx")
    for S in (-1, (1 << 24) + 1):
        _refused(lib, name, dict(make(P), S=S), f"S={S} out of range [0, 2^24]")
    for field in ("a", "b", "model", "ok"):
        _refused(lib, name, dict(make(P), **{field: None}), f"{name}: null device pointer")
    assert getattr(lib, name)(*dict(make(P), S=0, a=None, b=None, model=None, ok=None).values()) == _lib.SLAM_OK


@pytest.mark.parametrize("name", sorted(PER_CANDIDATE))
def test_per_candidate_entry_point_texts(built, name):
    from slamhip import _lib

    lib = _lib.load()
    make, cap, pointers = PER_CANDIDATE[name]
    _refused(lib, name, dict(make(P), ctx=None), f"{name}: null ctx")
    for kw in (dict(B=-1), dict(B=cap + 1), dict(M=-1), dict(M=(1 << 28) + 1)):
        a = dict(make(P), **kw)
        _refused(lib, name, a, f"bad sizes (B={a['B']}, M={a['M']})")
    for field in pointers:
        _refused(lib, name, dict(make(P), **{field: None}), f"{name}: null device pointer")
    assert getattr(lib, name)(*dict(make(P), B=0, off=None).values()) == _lib.SLAM_OK


def _raises(kind, text, fn, *args, **kw):
    with pytest.raises(kind) as err:
        fn(*args, **kw)
    assert type(err.value) is kind and str(err.value) == text, (fn.__name__, str(err.value))


def _wrappers():
    """(offsets form, batch form, a good candidate, how the wrapper names its candidates) of each estimator; the offsets forms
    are bound to take (array 1, array 2, offsets, **ransac arguments)."""
    import slamhip

    px, X = np.zeros((6, 2)), np.zeros((6, 3))
    return {
        "two_view": (lambda a, b, off, **kw: slamhip.find_essential_offsets(a, b, off, K, **kw),
                     lambda cands, **kw: slamhip.find_essential_batch(cands, K, **kw), (px, px), "pairs"),
        "pnp": (lambda a, b, off, **kw: slamhip.solve_pnp_ransac_offsets(a, b, off, K, **kw),
                lambda cands, **kw: slamhip.solve_pnp_ransac_batch(cands, K, **kw), (X, px), "candidates"),
        "homography": (lambda a, b, off, **kw: slamhip.find_homography_offsets(a, b, off, **kw),
                       lambda cands, **kw: slamhip.find_homography_batch(cands, **kw), (px, px), "pairs"),
        "sim3": (lambda a, b, off, **kw: slamhip.estimate_sim3_offsets(a, b, off, K, **kw),
                 lambda cands, **kw: slamhip.estimate_sim3_batch(cands, K, **kw), (X, X), "candidates"),
    }


@pytest.mark.parametrize("family", ["two_view", "pnp", "homography", "sim3"])
def test_wrapper_texts(family):
    offsets_form, batch_form, good, noun = _wrappers()[family]
    a, b = good
    gate = "chi2_gate" if family == "sim3" else "threshold"
    for form, args in ((offsets_form, (a, b, [0, 6])), (batch_form, ([good],))):
        _raises(TypeError, "hypotheses must be an integer", form, *args, hypotheses=2.5)
        _raises(TypeError, "hypotheses must be an integer", form, *args, hypotheses=True)
        _raises(ValueError, "hypotheses must be in [1, 1048576]", form, *args, hypotheses=0)
        _raises(ValueError, "hypotheses must be in [1, 1048576]", form, *args, hypotheses=(1 << 20) + 1)
        _raises(ValueError, "threshold must be positive", form, *args, **{gate: 0.0})
        _raises(ValueError, "threshold must be positive", form, *args, **{gate: np.nan})
        _raises(TypeError, "seed must be an integer", form, *args, seed=1.5)
    _raises(ValueError, "offsets must have B + 1 entries", offsets_form, a, b, [])
    _raises(ValueError, f"at most 65535 {noun} per call", offsets_form, a, b, np.zeros(65537, np.int32))
    _raises(ValueError, f"at most 65535 {noun} per call", batch_form, [good] * 65536)
    # an empty call comes back empty from both forms, with the mask as long as the arrays
    out = offsets_form(a, b, [0])
    mask = out[3] if family == "sim3" else out[1]
    assert mask.shape == (6,) and mask.dtype == bool and not mask.any()
    assert len(batch_form([])[0]) == 0


def test_wrapper_texts_of_the_arrays():
    import slamhip

    px, X = np.zeros((6, 2)), np.zeros((6, 3))
    w = _wrappers()
    for family, first, second in (("two_view", "px1", "px2"), ("homography", "px1", "px2")):
        off, batch = w[family][:2]
        _raises(ValueError, f"{first} must have shape [N,2], got (6, 3)", off, X, px, [0, 6])
        _raises(ValueError, f"{second} must have shape [N,2], got (6, 3)", off, px, X, [0, 6])
        _raises(TypeError, f"{first} must be numeric", off, [["a", "b"]], px, [0, 6])
        _raises(ValueError, "6 points in frame 1 but 5 in frame 2", off, px, px[:5], [0, 6])
        _raises(ValueError, "pair 1: expected (px1, px2)", batch, [(px, px), (px,)])
        _raises(ValueError, "pair 1 px2 must have shape [N,2], got (6, 3)", batch, [(px, px), (px, X)])
        _raises(ValueError, "pair 0: 6 points in frame 1 but 5 in frame 2", batch, [(px, px[:5])])
    off, batch = w["pnp"][:2]
    _raises(ValueError, "points must have shape [N,3], got (6, 2)", off, px, px, [0, 6])
    _raises(ValueError, "px must have shape [N,2], got (6, 3)", off, X, X, [0, 6])
    _raises(TypeError, "points must be numeric", off, [["a", "b", "c"]], px, [0, 6])
    _raises(ValueError, "6 points but 5 pixels", off, X, px[:5], [0, 6])
    _raises(ValueError, "candidate 1: expected (points, px)", batch, [(X, px), (X,)])
    _raises(ValueError, "candidate 0 points must have shape [N,3], got (6, 2)", batch, [(px, px)])
    _raises(ValueError, "candidate 0: 6 points but 4 pixels", batch, [(X, px[:4])])
    off, batch = w["sim3"][:2]
    _raises(ValueError, "X1 must have shape [N,3], got (6, 2)", off, px, X, [0, 6])
    _raises(ValueError, "X2 must have shape [N,3], got (6, 2)", off, X, px, [0, 6])
    _raises(ValueError, "6 points in frame 1 but 5 in frame 2", off, X, X[:5], [0, 6])
    _raises(ValueError, "sigma2 must have shape [6,2], got (5, 2)", off, X, X, [0, 6], sigma2=np.ones((5, 2)))
    _raises(TypeError, "sigma2 must be numeric", off, X, X, [0, 6], sigma2=[["a", "b"]] * 6)
    _raises(ValueError, "candidate 1: expected (X1, X2) or (X1, X2, sigma2)", batch, [(X, X), (X,)])
    _raises(ValueError, "candidate 0 X2 must have shape [N,3], got (6, 2)", batch, [(X, px)])
    _raises(ValueError, "candidate 0: 6 points in frame 1 but 5 in frame 2", batch, [(X, X[:5])])
    _raises(ValueError, "sigma2 must have shape [6,2], got (5, 2)", batch, [(X, X, np.ones((5, 2)))])
    # the refinement's list form, which concatenates the same way
    m13 = np.zeros((1, 13))
    _raises(ValueError, "candidate 0: expected (X1, X2, px1, px2) or (X1, X2, px1, px2, sigma2)", slamhip.optimize_sim3_batch, [(X, X, px)], m13, K)
    _raises(ValueError, "candidate 0: 6 points in frame 1 but 5 in frame 2", slamhip.optimize_sim3_batch, [(X, X[:5], px, px)], m13, K)
    _raises(ValueError, "candidate 0 px1 must have shape [6,2], got (5, 2)", slamhip.optimize_sim3_batch, [(X, X, px[:5], px)], m13, K)
    _raises(ValueError, "sigma2 must have shape [6,2], got (6, 3)", slamhip.optimize_sim3_batch, [(X, X, px, px, X)], m13, K)
    _raises(ValueError, "at most 65535 candidates per call", slamhip.optimize_sim3_offsets, X, X, px, px, np.zeros(65537, np.int32),
            np.zeros((65536, 13)), K)
    _raises(ValueError, "at most 16777216 candidates per call", slamhip.fit_sim3_offsets, X, X, np.zeros((1 << 24) + 2, np.int32))
    # intrinsics, shared by all of them
    _raises(ValueError, "intrinsics must be a 3x3 camera matrix or (fx, fy, cx, cy), got shape (2, 2)", slamhip.find_essential_offsets, px, px,
            [0, 6], np.eye(2))
    _raises(ValueError, "focal lengths must be positive and intrinsics finite", slamhip.solve_pnp_ransac_offsets, X, px, [0, 6], (0.0, 1.0, 0.0, 0.0))
    _raises(ValueError, "focal lengths must be positive and intrinsics finite", slamhip.estimate_sim3_offsets, X, X, [0, 6], (1.0, 1.0, np.inf, 0.0))


def test_loop_edge_builder_texts():
    import slamhip

    R, t, T = np.tile(np.eye(3), (1, 1, 1)), np.zeros((1, 3)), np.tile(np.eye(4)[:3], (1, 1, 1))
    maps, srt = np.tile(np.eye(4), (3, 1, 1)), (np.ones(1), np.tile(np.eye(3), (1, 1, 1)), np.zeros((1, 3)))
    builders = {
        "two_view": lambda pairs=((0, 1),), n=(30,), **kw: slamhip.loop_edges_from_two_view(pairs, R, t, n, **kw),
        "pnp": lambda pairs=((0, 1),), n=(30,), **kw: slamhip.loop_edges_from_pnp(pairs, T, n, maps, **kw),
        "sim3": lambda pairs=((0, 1),), n=(30,), **kw: slamhip.loop_edges_from_sim3(pairs, srt, n, **kw),
        "sim3_graph": lambda pairs=((0, 1),), n=(30,), **kw: slamhip.sim3_edges_from_sim3(pairs, srt, n, **kw),
    }
    sigmas = {"two_view": "min_inliers >= 1 and positive sigmas", "pnp": "min_inliers >= 1 and positive sigmas",
              "sim3": "min_inliers >= 1, positive sigmas and max_log_scale >= 0", "sim3_graph": "min_inliers >= 1 and positive sigmas"}
    counts = {"two_view": "2 pairs but 1 rotations, 1 translations, 1 inlier counts", "pnp": "2 pairs but 1 poses and 1 inlier counts",
              "sim3": "2 pairs but 1 scales, 1 rotations, 1 translations and 1 inlier counts", "sim3_graph": "2 pairs but 1 models and 1 inlier counts"}
    for name, build in builders.items():
        _raises(ValueError, "pairs must be integers of shape [B,2], got float64 (1, 2)", build, pairs=[[0.0, 1.0]])
        _raises(ValueError, "pairs must be integers of shape [B,2], got int64 (1, 3)", build, pairs=np.array([[0, 1, 2]], np.int64))
        _raises(ValueError, counts[name], build, pairs=[[0, 1], [1, 2]])
        for kw in (dict(min_inliers=0), dict(rotation_sigma=0.0), dict(translation_sigma=-1.0)):
            _raises(ValueError, sigmas[name], build, **kw)
        edges, meas, info = build(n=(40,), min_inliers=20, rotation_sigma=0.1, translation_sigma=0.5)[:3]
        assert edges.tolist() == [[0, 1]] and edges.dtype == np.int32
        want = [2.0 / 0.1 ** 2] * 3 + ([0.0] * 3 if name == "two_view" else [2.0 / 0.5 ** 2] * 3)
        if name == "sim3_graph":
            want.append(2.0 / 0.05 ** 2)
        assert np.array_equal(info[0], np.diag(want))                   # inliers / min_inliers / sigma^2, to the bit
        assert build(n=(19,), min_inliers=20)[0].shape == (0, 2) and build(pairs=[[1, 1]])[0].shape == (0, 2)
    _raises(ValueError, sigmas["sim3_graph"], builders["sim3_graph"], scale_sigma=0.0)
    _raises(ValueError, sigmas["sim3"], builders["sim3"], max_log_scale=-1.0)
    _raises(ValueError, "pair index outside the 3 map poses", builders["pnp"], pairs=[[0, 3]])
    _raises(ValueError, "negative pair index", builders["sim3"], pairs=[[0, -1]])
    _raises(ValueError, "negative pair index", builders["sim3_graph"], pairs=[[0, -1]])
    _raises(ValueError, "models must be (s [B], R [B,3,3], t [B,3])", slamhip.loop_edges_from_sim3, [[0, 1]], srt[:2], [30])
    _raises(ValueError, "models must be (s [B], R [B,3,3], t [B,3])", slamhip.sim3_edges_from_sim3, [[0, 1]], srt[:2], [30])
    scaled = slamhip.loop_edges_from_two_view([[0, 1]], R, t, [40], min_inliers=20, rotation_sigma=0.1, scale=2.0, translation_sigma=0.5)[2]
    assert np.array_equal(scaled[0], np.diag([2.0 / 0.1 ** 2] * 3 + [1.0 / 0.5 ** 2] * 3))
