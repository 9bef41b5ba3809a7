"""Maker of tests/golden/geometry_parent.json: what the four batched RANSAC estimators (csrc/two_view.hip, pnp.hip,
homography.hip, sim3.hip) return, bit for bit, at the commit BEFORE csrc/geometry_common.h gave them one copy of the sampler,
the Jacobi sweeps, the triangulation, the cheirality test, the range clamp and the model keys.
tests/test_geometry_parent_cpu.py replays the `twin` section (the host twins, no GPU) and tests/test_geometry_parent_gpu.py the
`gpu` section (the public slamhip API), both through record_case(), and compare.  Only the public API, the twin modules and
the ref modules' generators are used, so this file runs unchanged on either side of the change.

One case per estimator and section; per case:
  solver    the minimal solver on S = 65 samples (one full 64-lane block and a block with 63 spare lanes): 53 samples of the
            ref module's generator and 12 degenerate ones (repeated point, flat triangle, NaN / inf / 1e150)
  ransac    one call of B = 4 candidates of SAMPLE - 1, SAMPLE (every draw walks the duplicate-rejection loop), 256 and 257
            (one LDS chunk, and one past it) noisy matches with outliers, for H in 1, 64, 257 (a second block of hypotheses on
            spare lanes) and seeds 0 and 2^63 + 1 (the generator's high word)
  clamp     gpu only (a twin takes one candidate and no offsets): the same call at H = 64 with an offsets table that starts
            below 0, runs past M and steps backwards, and the index-error count it leaves; every other entry point that
            takes offsets is called on that table too
  what follows the RANSAC on its winners: recover_pose (with and without the vote) and triangulate for two_view; decompose
            and model_score for homography, and the three pure-rotation scenes of tests/two_view_ref.py; refit for sim3 on
            candidates of 0, 2, 3 and 257 points with and without a mask, with fix_scale both ways
Arrays are recorded as SHA-256 of their raw bytes, integer stats as they are.

Run at that commit from the repository root:  python tests/golden/make_geometry_parent.py --section twin --commit <hash>
and, on a GPU,                                python tests/golden/make_geometry_parent.py --section gpu --commit <hash>
(each keeps the other section of an existing fixture; --out writes the merged fixture somewhere else)."""
import argparse
import ctypes
import hashlib
import json
import os
import shutil
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
for p in (TESTS, ROOT, os.path.join(ROOT, "slam-experiments_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
import homography_ref as hr  # noqa: E402
import pnp_ref as pr  # noqa: E402
import sim3_ref as sr  # noqa: E402
import two_view_ref as tr  # noqa: E402

FIXTURE = os.path.join(HERE, "geometry_parent.json")
PARENT = "fd0e53a"
SECTIONS = ("twin", "gpu")
ESTIMATORS = ("two_view", "pnp", "homography", "sim3")
CASES = {s: tuple(f"{s}/{e}" for e in ESTIMATORS) for s in SECTIONS}
K = tr.EUROC
HS = (1, 64, 257)
SEEDS = (0, (1 << 63) + 1)
SEED = 4711
S_RANDOM, S_TOTAL = 53, 65


def toolchain():
    """the compilers behind the two sections: hipcc (the library) and g++ (the twins)"""
    out = []
    for cc in (shutil.which("hipcc") or "/opt/rocm/bin/hipcc", "g++"):
        try:
            out.append(subprocess.run([cc, "--version"], capture_output=True, text=True, check=True).stdout.strip().splitlines()[0])
        except (OSError, subprocess.CalledProcessError, IndexError) as err:
            out.append(f"{cc} --version failed: {err}")
    return "; ".join(out)


def fig(*vals):
    """one figure: small integer arrays as they are, everything else as the SHA-256 of its bytes"""
    out = []
    for v in vals:
        a = np.ascontiguousarray(v)
        if a.dtype.kind in "iu" and a.size <= 64:
            out.append(str(a.reshape(-1).tolist()))
        else:
            out.append(hashlib.sha256((a.astype(np.uint8) if a.dtype == bool else a).tobytes()).hexdigest())
    return " ".join(out)


def cat(cands):
    """candidates (tuples of arrays of one length each) -> (the concatenated arrays, offsets int32 [B + 1])"""
    off = np.cumsum([0] + [len(c[0]) for c in cands]).astype(np.int32)
    return [np.ascontiguousarray(np.concatenate([c[i] for c in cands])) for i in range(len(cands[0]))], off


def bad_offsets(off):
    """below 0, past M, backwards: the clamped slices are [0, off[1]), [off[1], off[2]), [off[2], M) and an empty one"""
    M = int(off[-1])
    return np.array([-3, off[1], off[2], M + 5, off[2] + 10], np.int32)


def index_errors(ctx):
    from slamhip._lib import check

    n = ctypes.c_int64(-1)
    check(ctx.lib.slam_index_errors(ctx.handle, ctypes.byref(n)))
    return int(n.value)


def each(off, fn):
    """fn(slice) per candidate, the results stacked field by field (1-D per-match fields concatenated)"""
    res = [fn(slice(int(off[b]), int(off[b + 1]))) for b in range(len(off) - 1)]
    return [np.concatenate(f) if f[0].dtype in (bool, np.uint8) else np.stack(f) for f in map(list, zip(*res))]


def sweep(out, run):
    for H in HS:
        for seed in SEEDS:
            out[f"ransac/H{H}/seed{seed}"] = fig(*run(H, seed))


# ---------------------------------------------------------------------------------------------------- two_view
def two_view_case(ctx):
    from oracle import oracle

    gpu = ctx is not None
    if gpu:
        from slamhip import two_view as tv
    out = {}
    x1, x2, _ = tr.make_samples(SEED, S_RANDOM, 0.5)
    for sc in (tr.scenes_duplicates()[0], tr.scenes_collinear()[1], tr.scenes_non_finite()[1]):
        _, a, b = tr.family_samples(sc, 0, 4)
        x1, x2 = np.concatenate([x1, a]), np.concatenate([x2, b])
    assert len(x1) == S_TOTAL
    out["solver"] = fig(*(tv.fivepoint_arrays(x1, x2, ctx) if gpu else oracle.tv_twin_solve(x1, x2)))

    rng = np.random.default_rng([SEED, 1])
    (px1, px2), off = cat([(sc["px1"], sc["px2"]) for sc in (tr.make_scene(rng, n, 0.5, 0.2) for n in (4, 5, 256, 257))])

    def ransac(H, seed, o=off):
        if gpu:
            return tv.find_essential_offsets(px1, px2, o, K, H, 1.0, seed, ctx)
        return each(o, lambda s: oracle.tv_twin_ransac(px1[s], px2[s], K, H, 1.0, seed))

    def recover(E, inl, o=off):
        if gpu:
            return tv.recover_pose_offsets(E, px1, px2, o, K, inl, 50.0, ctx)
        E = np.asarray(E).reshape(-1, 9)
        res = [oracle.tv_twin_recover_pose(E[b], px1[s], px2[s], K, None if inl is None else inl[s])[:3]
               for b, s in enumerate(slice(int(o[b]), int(o[b + 1])) for b in range(len(o) - 1))]
        return np.stack([r[0] for r in res]), np.concatenate([r[1] for r in res]), np.stack([r[2] for r in res])

    sweep(out, ransac)
    E, mask, _ = ransac(64, 0)
    pose, good, st = recover(E, mask)
    out["recover_pose/vote"] = fig(pose, good, st)
    out["recover_pose/all"] = fig(*recover(E, None))
    s = slice(int(off[3]), int(off[4]))
    P1, a, b = np.eye(4)[:3], tr.normalise(px1[s], K), tr.normalise(px2[s], K)
    out["triangulate"] = fig(*(tv.triangulate_arrays(P1, pose[3], a, b, ctx) if gpu else oracle.tv_twin_triangulate(P1, pose[3], a, b)))
    if gpu:
        index_errors(ctx)
        bad = bad_offsets(off)
        Eb, mb, sb = ransac(64, 0, bad)
        out["clamp/ransac"] = fig(Eb, mb, sb) + f" errors {index_errors(ctx)}"
        out["clamp/recover_pose"] = fig(*recover(Eb, mb, bad)) + f" errors {index_errors(ctx)}"
    return out


# ---------------------------------------------------------------------------------------------------- pnp
def pnp_case(ctx):
    import pnp_twin as tw

    gpu = ctx is not None
    if gpu:
        from slamhip import pnp
    out = {}
    X, x, _, _ = pr.make_samples(S_RANDOM, SEED)
    Xe, xe = pr.solver_edge_samples()
    X, x = np.concatenate([X, Xe]), np.concatenate([x, xe])
    assert len(X) == S_TOTAL
    out["solver"] = fig(*(pnp.p3p_arrays(X, x, ctx) if gpu else tw.p3p(X, x)))

    rng = np.random.default_rng([SEED, 2])
    (P, px), off = cat([(sc["X"], sc["px"]) for sc in (pr.make_scene(rng, n, 0.5, 0.2) for n in (2, 3, 256, 257))])

    def ransac(H, seed, o=off):
        if gpu:
            return pnp.solve_pnp_ransac_offsets(P, px, o, K, H, 8.0, seed, ctx)
        return each(o, lambda s: tw.ransac(P[s], px[s], K, H, 8.0, seed))

    sweep(out, ransac)
    if gpu:
        index_errors(ctx)
        out["clamp/ransac"] = fig(*ransac(64, 0, bad_offsets(off))) + f" errors {index_errors(ctx)}"
    return out


# ---------------------------------------------------------------------------------------------------- homography
HG_KEYS = ("pose_all", "normal_all", "count", "pose", "sv", "good", "stats")


def _hg_degenerate():
    p1 = np.array([[100.0, 100], [600, 120], [580, 400], [90, 380]])
    p2 = np.array([[120.0, 90], [610, 140], [560, 420], [110, 360]])
    A, B = np.tile(p1, (12, 1, 1)), np.tile(p2, (12, 1, 1))
    A[0, 2] = A[0, 0]; B[1, 3] = B[1, 1]                                # a repeated point in either image
    A[2, 2] = 0.5 * (A[2, 0] + A[2, 1]); B[3, :, 1] = 3.0 * B[3, :, 0] + 1.0    # a flat triangle; all four on a line
    B[4, [0, 1]] = B[4, [1, 0]]                                         # a triangle turned over
    A[5, 1, 0] = np.nan; B[6, 3, 1] = -np.inf; A[7, 0] = [1e150, -1e150]; A[8] = A[8, 0]
    A[9] *= 1e90; B[9] *= 1e-90                                         # inside the range: solved
    B[10, 2, 0] = np.nan
    return A, B


def homography_case(ctx):
    import hg_twin as tw
    from oracle import oracle

    gpu = ctx is not None
    if gpu:
        from slamhip import homography as hg
        from slamhip import two_view as tv
    out = {}
    p1, p2, _ = hr.fourpoint_samples(SEED, S_RANDOM)
    A, B = _hg_degenerate()
    p1, p2 = np.concatenate([p1, A]), np.concatenate([p2, B])
    assert len(p1) == S_TOTAL
    if gpu:
        Hs, ok = hg.fourpoint_homography_arrays(p1, p2, ctx)
    else:
        Hs, ok = tw.fourpoint(p1, p2)
    out["solver"] = fig(Hs.reshape(-1, 9), np.asarray(ok).astype(np.int32))

    def essential(px1, px2, o):
        if gpu:
            return tv.find_essential_offsets(px1, px2, o, K, 64, 1.0, 0, ctx)[0]
        return each(o, lambda s: oracle.tv_twin_ransac(px1[s], px2[s], K, 64, 1.0, 0))[0]

    def ransac(px1, px2, o, H, seed):
        if gpu:
            return hg.find_homography_offsets(px1, px2, o, H, 3.0, seed, ctx)
        return each(o, lambda s: tw.ransac(px1[s], px2[s], H, 3.0, seed))

    def decompose(Hm, px1, px2, o, inl):
        if gpu:
            d = hg.decompose_homography_offsets(Hm, px1, px2, o, K, inl, 50.0, ctx)
            return [d[k] for k in HG_KEYS]
        Hm = np.asarray(Hm).reshape(-1, 9)
        res = [tw.decompose(px1[s], px2[s], K, Hm[b], None if inl is None else inl[s])
               for b, s in enumerate(slice(int(o[b]), int(o[b + 1])) for b in range(len(o) - 1))]
        return [np.concatenate([r[k] for r in res]) if k == "good" else np.stack([r[k] for r in res]) for k in HG_KEYS]

    def score(Hm, E, px1, px2, o):
        if gpu:
            return hg.model_scores_offsets(Hm, E, px1, px2, o, K, 1.0, ctx)
        Hm, E = np.asarray(Hm).reshape(-1, 9), np.asarray(E).reshape(-1, 9)
        res = [tw.model_score(px1[s], px2[s], K, Hm[b], E[b])
               for b, s in enumerate(slice(int(o[b]), int(o[b + 1])) for b in range(len(o) - 1))]
        return np.stack([r[0] for r in res]), np.array([r[1] for r in res])

    (px1, px2), off = cat([(sc["px1"], sc["px2"]) for sc in (hr.scenes_planar_noisy(SEED, n)[1] for n in (3, 4, 256, 257))])
    sweep(out, lambda H, seed: ransac(px1, px2, off, H, seed))
    Hm, mask, _ = ransac(px1, px2, off, 64, 0)
    E = essential(px1, px2, off)
    out["decompose/vote"] = fig(*decompose(Hm, px1, px2, off, mask))
    out["decompose/all"] = fig(*decompose(Hm, px1, px2, off, None))
    out["model_score"] = fig(*score(Hm, E, px1, px2, off))
    (q1, q2), roff = cat([(sc["px1"], sc["px2"]) for sc in tr.scenes_pure_rotation(0, 200)])
    Hr, rmask, rst = ransac(q1, q2, roff, 64, 0)
    out["pure_rotation/ransac"] = fig(Hr, rmask, rst)
    out["pure_rotation/decompose"] = fig(*decompose(Hr, q1, q2, roff, rmask))
    if gpu:
        index_errors(ctx)
        bad = bad_offsets(off)
        Hb, mb, sb = ransac(px1, px2, bad, 64, 0)
        out["clamp/ransac"] = fig(Hb, mb, sb) + f" errors {index_errors(ctx)}"
        out["clamp/decompose"] = fig(*decompose(Hb, px1, px2, bad, mb)) + f" errors {index_errors(ctx)}"
        out["clamp/model_score"] = fig(*score(Hb, E, px1, px2, bad)) + f" errors {index_errors(ctx)}"
    return out


# ---------------------------------------------------------------------------------------------------- sim3
def _sim3_degenerate():
    X1, X2, _ = sr.solver_samples(12, sr.SEED + 3)
    X1[0, 1] = X1[0, 0]; X2[1, 2] = X2[1, 0]                            # a repeated point in either set
    X1[2, 2] = X1[2, 0] + 3.0 * (X1[2, 1] - X1[2, 0]); X2[3, 2] = X2[3, 0] - 0.5 * (X2[3, 1] - X2[3, 0])    # flat triangles
    X1[4] = X1[4, 0]; X2[4] = X2[4, 0]
    X1[5, 0, 1] = np.nan; X2[6, 1, 0] = np.nan; X1[7, 2, 2] = np.inf; X2[8, 0, 1] = -np.inf; X1[9, 1, 0] = 1e150; X2[10, 2, 1] = 1e150
    return X1, X2


def sim3_case(ctx):
    import sim3_twin as tw

    gpu = ctx is not None
    if gpu:
        from slamhip import sim3 as s3
    out = {}
    X1, X2, _ = sr.solver_samples(S_RANDOM, SEED)
    A, B = _sim3_degenerate()
    X1, X2 = np.concatenate([X1, A]), np.concatenate([X2, B])
    assert len(X1) == S_TOTAL
    for fix in (False, True):
        out[f"solver/fix{int(fix)}"] = (fig(*s3.sim3_threepoint_arrays(X1, X2, fix, ctx)) if gpu else
                                        fig(*tw.split(tw.threepoint(X1, X2, fix)[0]), tw.threepoint(X1, X2, fix)[1]))

    rng = np.random.default_rng([SEED, 4])
    (P1, P2), off = cat([(sc["X1"], sc["X2"]) for sc in (sr.make_scene(rng, n, 1.3, 0.001, 0.2) for n in (2, 3, 256, 257))])
    sigma2 = rng.uniform(0.5, 2.0, (len(P1), 2))

    def ransac(H, seed, o=off, sg=None, fix=False):
        if gpu:
            return s3.estimate_sim3_offsets(P1, P2, o, K, H, sr.CHI2, sg, fix, seed, False, ctx)[:5]
        model, mask, st = each(o, lambda s: tw.ransac(P1[s], P2[s], K, H, sr.CHI2, seed, None if sg is None else sg[s], fix))
        return tw.split(model) + (mask, st)

    def refit(A1, A2, o, mask, fix):
        if gpu:
            return s3.fit_sim3_offsets(A1, A2, o, mask, fix, ctx)
        res = [tw.refit(A1[s], A2[s], None if mask is None else mask[s], fix)
               for s in (slice(int(o[b]), int(o[b + 1])) for b in range(len(o) - 1))]
        return tw.split(np.stack([r[0] for r in res])) + (np.stack([r[1] for r in res]),)

    sweep(out, ransac)
    out["ransac/sigma2/fix1"] = fig(*ransac(64, 0, off, sigma2, True))
    mask = ransac(64, 0)[3]
    out["refit/ransac_vote"] = fig(*refit(P1, P2, off, mask, False))
    (Q1, Q2), roff = cat([(sc["X1"], sc["X2"]) for sc in (sr.make_scene(rng, n, 0.7, 0.001) for n in (0, 2, 3, 257))])
    rmask = rng.random(len(Q1)) < 0.7
    for fix in (False, True):
        out[f"refit/all/fix{int(fix)}"] = fig(*refit(Q1, Q2, roff, None, fix))
        out[f"refit/mask/fix{int(fix)}"] = fig(*refit(Q1, Q2, roff, rmask, fix))
    if gpu:
        index_errors(ctx)
        bad = bad_offsets(off)
        res = ransac(64, 0, bad)
        out["clamp/ransac"] = fig(*res) + f" errors {index_errors(ctx)}"
        out["clamp/refit"] = fig(*refit(P1, P2, bad, res[3], False)) + f" errors {index_errors(ctx)}"
    return out


RUN = dict(two_view=two_view_case, pnp=pnp_case, homography=homography_case, sim3=sim3_case)


def record_case(case, ctx=None):
    """every recorded figure of one case as {name: str}; the gpu section needs a context, the twin section takes none"""
    section, estimator = case.split("/")
    assert (ctx is not None) == (section == "gpu"), case
    with np.errstate(all="ignore"):
        return RUN[estimator](ctx)


def compare(case, got, want, recorded):
    """the replaying tests' assertion: every figure equal, the differing ones printed with what both sides were made with"""
    differing = sorted(k for k in set(got) | set(want) if got.get(k) != want.get(k))
    for k in differing:
        print(f"{case} {k}\n  recorded {want.get(k)}\n  got      {got.get(k)}")
    assert not differing, (f"{case}: {len(differing)} of {len(want)} figures differ from the parent's: {differing}\n"
                           f"recorded with: numpy {recorded['numpy']}, {recorded['toolchain']}\n"
                           f"running with:  numpy {np.__version__}, {toolchain()}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--section", choices=SECTIONS, required=True)
    ap.add_argument("--commit", required=True, help="the commit this tree is at (the fixture records it)")
    ap.add_argument("--out", default=FIXTURE)
    args = ap.parse_args()
    ctx = None
    if args.section == "gpu":
        import slamhip

        ctx = slamhip.default_context()
    doc = {}
    if os.path.exists(FIXTURE):
        with open(FIXTURE) as f:
            doc = json.load(f)
    cases = {case: record_case(case, ctx) for case in CASES[args.section]}
    doc[args.section] = {"commit": args.commit, "toolchain": toolchain(), "numpy": np.__version__, "cases": cases}
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {args.out}: section {args.section}, {len(cases)} cases, {sum(len(c) for c in cases.values())} figures")


if __name__ == "__main__":
    main()
