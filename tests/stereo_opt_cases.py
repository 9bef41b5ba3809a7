"""Scenes of the stereo / level-weighted adjustments (tests/test_stereo_opt_cpu.py, tests/test_stereo_opt_gpu.py): frames for
the pose optimisation, the windows of tests/ba_sparse_ref.py with a third measurement and pyramid levels, and a local window
with planted outliers and an unobservable monocular scale.  Built from seeds, by index rules, never from a result."""
import numpy as np

import ba_sparse_ref as R
from oracle import oracle

FX, FY, CX, CY = R.INTR
BASELINE = 0.11
BF = FX * BASELINE
CAM = (FX, FY, CX, CY, BF)
SCALE = 1.2 ** np.arange(8)                 # ORB-SLAM's pyramid: sigma of a keypoint of level l is SCALE[l] pixels
STAGE = 512                                 # SLAM_POSE_STEREO_STAGE
POSE_SCENES = {"o12": (12, 4), "o200": (200, 228), "stage": (STAGE, 7), "stage+1": (STAGE + 1, 8)}


def project3(T, X):
    """(u, v, u_right) of points X [n,3] under T 4x4."""
    pc = X @ T[:3, :3].T + T[:3, 3]
    u = FX * pc[:, 0] / pc[:, 2] + CX
    return np.stack([u, FY * pc[:, 1] / pc[:, 2] + CY, u - BF / pc[:, 2]], 1)


def pose_frame(seed, O, planted=True, noise=0.6):
    """One frame of O edges: level i % 8, information 1 / SCALE[level]^2, stereo for even i, pixel noise `noise` * SCALE[level].
    Planted (by index): i % 7 == 3 a gross pixel outlier (i = 3 monocular, i = 10 stereo, ..), i % 22 == 8 a stereo edge whose
    u_right alone is off, i == 5 and i % 97 == 50 switched off (information 0, a wild measurement).
    -> dict(T, T_init, X, meas3, info, level, bad bool [O], off bool [O])."""
    rng = np.random.default_rng(seed)
    T, X = R.scene(rng, 1, O)
    T = T[0]
    i = np.arange(O)
    level = i % 8
    sig = SCALE[level]
    meas3 = project3(T, X) + rng.normal(0, noise, (O, 3)) * sig[:, None]
    meas3[i % 2 == 1, 2] = np.nan
    bad, off = np.zeros(O, bool), np.zeros(O, bool)
    if planted:
        gross = i % 7 == 3
        meas3[gross, :2] += rng.uniform(40, 120, (int(gross.sum()), 2)) * rng.choice([-1, 1], (int(gross.sum()), 2))
        right = (i % 22 == 8)
        meas3[right, 2] += 25.0 * sig[right]
        off = (i == 5) | (i % 97 == 50)
        meas3[off, :2] += 500.0
        bad = (gross | right) & ~off
    info = np.where(off, 0.0, 1.0 / (sig * sig))
    T_init = oracle.se3_exp_np(rng.normal(0, 0.02, 6)) @ T
    return dict(T=T, T_init=T_init, X=X, meas3=meas3, info=info, level=level, bad=bad, off=off)


_frames = {}


def pose_scene(name):
    """A named scene of POSE_SCENES, built once."""
    if name not in _frames:
        O, seed = POSE_SCENES[name]
        _frames[name] = pose_frame(seed, O)
    return _frames[name]


def mono_frame(seed, O):
    """The frame of tests/test_optimize_gpu.py::test_device_lm_matches_oracle: unit information, no u_right, int-truncated
    pixels, every seventh edge a gross outlier."""
    rng = np.random.default_rng(seed)
    T, X = R.scene(rng, 1, O)
    meas = project3(T[0], X)[:, :2] + rng.normal(0, 0.4, (O, 2))
    bad = np.arange(0, O, 7)
    meas[bad] += rng.uniform(40, 120, (len(bad), 2)) * rng.choice([-1, 1], (len(bad), 2))
    meas = meas.astype(np.int32).astype(np.float64)
    T_init = oracle.se3_exp_np(rng.normal(0, 0.02, 6)) @ T[0]
    return dict(T=T[0], T_init=T_init, X=X, meas=meas, meas3=np.c_[meas, np.full(O, np.nan)], info=np.ones(O), bad=bad)


def depth_shift_frame(seed=31, O=160, shift=1.5, cone=0.005):
    """A frame whose map was shifted along the optical axis and scaled so that monocular reprojection does not see it: the
    camera sits at the origin looking down z, the true points lie in a narrow cone (|x|, |y| <= `cone` * z, 7..9 m deep) and the
    MAP holds every point pushed `shift` metres deeper along its own viewing ray (for the cone: the slab moved by `shift` and
    scaled by 1 + shift / z).  At the identity pose every monocular residual is pure noise, whatever `shift`; the disparities
    say the points are `shift` closer.  A camera that moves `shift` forward meets the measured depths and changes the
    monocular reprojection by fx (x / z) (shift / z) only - second order in the cone.  The metric answer is |t| = shift.
    Noise sigma_d = 0.3 px on all three measurements (times SCALE[level], levels 0..3).
    -> dict(T_init, X (the map), meas3, info, shift, sigma_d, depth)."""
    rng = np.random.default_rng(seed)
    Z = rng.uniform(7.0, 9.0, O)
    X = np.c_[rng.uniform(-cone, cone, O) * Z, rng.uniform(-cone, cone, O) * Z, Z]
    level = np.arange(O) % 4
    sig = SCALE[level]
    meas3 = project3(np.eye(4), X) + rng.normal(0, 0.3, (O, 3)) * sig[:, None]
    Xmap = X * ((Z + shift) / Z)[:, None]
    return dict(T_init=np.eye(4), X=Xmap, meas3=meas3, info=1.0 / (sig * sig), level=level, shift=shift, sigma_d=0.3, depth=float(Z.mean()))


def stereo_window(w, seed):
    """A window of ba_sparse_ref (case_edges, case_hub) with u_right given to about half of the observations and levels 0..7:
    (meas3 [O,3] whose first two columns are the window's own pixels, info [O])."""
    rng = np.random.default_rng(seed)
    O = len(w["op"])
    pc = np.einsum("oij,oj->oi", w["T"][w["op"], :3, :3], w["X"][w["ol"]]) + w["T"][w["op"], :3, 3]
    level = rng.integers(0, 8, O)
    ur = FX * pc[:, 0] / pc[:, 2] + CX - BF / pc[:, 2] + rng.normal(0, 0.3, O)
    ur[rng.random(O) < 0.5] = np.nan
    return np.c_[w["meas"], ur], 1.0 / (SCALE[level] * SCALE[level])


def local_window(seed=77, K=12, L=300, scale=1.1):
    """A local window for LocalBundleAdjustment's schedule: K = 12 poses of which 0 and 1 are fixed and share ONE camera centre
    (they differ by a rotation), so that monocular edges leave the scale of the rest free; about L points, each seen by 3 to 6
    poses; levels 0..3, noise 0.3 * SCALE[level].  The start state is the truth scaled by `scale` about that centre (points and
    the centres of the free poses: monocular reprojection unchanged), plus a small perturbation.  Planted: observations
    o % 29 == 4 gross pixel outliers (both kinds occur), o % 41 == 9 with u_right a stereo outlier in u_right alone, and point
    7 starts behind pose 2's camera.
    -> dict(T0, X0, op, ol, meas3, info, fixed, T, X, planted bool [O], scale)."""
    from scipy.spatial.transform import Rotation

    rng = np.random.default_rng(seed)
    T = np.tile(np.eye(4), (K, 1, 1))
    T[:, :3, :3] = Rotation.from_rotvec(rng.uniform(-0.12, 0.12, (K, 3))).as_matrix()
    centre = rng.uniform(-0.6, 0.6, (K, 3))
    centre[0] = centre[1] = 0.0
    T[:, :3, 3] = -np.einsum("kij,kj->ki", T[:, :3, :3], centre)
    X = np.c_[rng.uniform(-3, 3, (L, 2)), rng.uniform(6, 12, L)]
    op, ol = [], []
    for l in range(L):
        seen = rng.choice(K, int(rng.integers(3, 7)), replace=False)
        op += sorted(seen.tolist())
        ol += [l] * len(seen)
    perm = rng.permutation(len(op))
    op, ol = np.asarray(op, np.int32)[perm], np.asarray(ol, np.int32)[perm]
    O = len(op)
    level = rng.integers(0, 4, O)
    sig = SCALE[level]
    pc = np.einsum("oij,oj->oi", T[op, :3, :3], X[ol]) + T[op, :3, 3]
    u = FX * pc[:, 0] / pc[:, 2] + CX
    meas3 = np.stack([u, FY * pc[:, 1] / pc[:, 2] + CY, u - BF / pc[:, 2]], 1) + rng.normal(0, 0.3, (O, 3)) * sig[:, None]
    meas3[rng.random(O) < 0.5, 2] = np.nan
    o = np.arange(O)
    gross = o % 29 == 4
    meas3[gross, :2] += rng.uniform(40, 90, (int(gross.sum()), 2)) * rng.choice([-1, 1], (int(gross.sum()), 2))
    right = (o % 41 == 9) & ~np.isnan(meas3[:, 2])
    meas3[right, 2] += 30.0 * sig[right]
    T0, X0 = T.copy(), X * scale
    for k in range(2, K):
        Tk = np.eye(4)
        Tk[:3, :3] = T[k, :3, :3]
        Tk[:3, 3] = -T[k, :3, :3] @ (centre[k] * scale)
        T0[k] = oracle.se3_exp_np(rng.normal(0, 0.003, 6)) @ Tk
    X0 += rng.normal(0, 0.02, X0.shape)
    X0[7] = centre[2] * scale - 0.8 * T[2, 2, :3]               # 0.8 m behind pose 2's camera along its optical axis
    return dict(T0=T0, X0=X0, op=op, ol=ol, meas3=meas3, info=1.0 / (sig * sig), fixed=(0, 1), T=T, X=X, planted=gross | right, scale=scale,
                centre=centre)


def window_scale(T, centre_true):
    """The scale of a state against the truth: the ratio of the free poses' camera-centre norms (about the fixed centre 0)."""
    c = -np.einsum("kji,kj->ki", T[2:, :3, :3], T[2:, :3, 3])
    return float(np.linalg.norm(c) / np.linalg.norm(centre_true[2:]))
