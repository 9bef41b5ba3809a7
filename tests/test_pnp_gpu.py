"""Absolute pose on the GPU (slam_pnp_*) against the host twin of csrc/pnp.hip (tests/pnp_twin.py), BIT FOR BIT: the file is
compiled with contraction off and uses + - * / sqrt only, so the device must give what the host build of the same source
gives; what the twin itself is worth is tests/test_pnp_cpu.py's business (numpy solver on another route, 16 x yardsticks).
Then batching, the kernel's own boundaries, the refinement and one relative timing."""
import ctypes

import numpy as np
import pytest

import pnp_ref as ref
import pnp_twin as tw

pytestmark = pytest.mark.gpu
K = ref.EUROC
CHUNK = 256                                    # PNP_CHUNK of csrc/pnp.hip: correspondences staged in LDS at a time


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------ device == twin
def test_solver_is_the_twin_bit_for_bit(gpu_ctx):
    import slamhip

    X, x, _, _ = ref.make_samples(2000)
    pose, n = slamhip.p3p_arrays(X, x, ctx=gpu_ctx)
    pt, nt = tw.p3p(X, x)
    assert np.array_equal(n, nt) and np.array_equal(pose.view(np.uint64), pt.view(np.uint64))
    assert n.min() >= 1 and np.isfinite(pose).all()
    p1, n1 = slamhip.p3p_arrays(X[7], x[7], ctx=gpu_ctx)                # one sample, [3,3] / [3,2]
    assert np.array_equal(p1[0], pose[7]) and n1[0] == n[7]


@pytest.fixture(scope="module")
def scenes():
    return ref.end_to_end_scenes()


def test_ransac_is_the_twin_bit_for_bit_on_the_end_to_end_scenes(gpu_ctx, scenes):
    import slamhip

    poses, masks, counts, st, _ = slamhip.solve_pnp_ransac_batch([(sc["X"], sc["px"]) for _, sc in scenes], K, refine=False, ctx=gpu_ctx)
    for i, (share, sc) in enumerate(scenes):
        pt, mt, stt = tw.ransac(sc["X"], sc["px"], K, 256, 8.0, 0)
        assert np.array_equal(poses[i].view(np.uint64), pt.view(np.uint64)) and np.array_equal(masks[i], mt) and np.array_equal(st[i], stt), i
        assert counts[i] == masks[i].sum() == st[i, 0]
        rot, tr = ref.pose_errors(poses[i], sc)
        print(f"outliers {share}: rot {rot:.4f} deg, dt {tr:.4f}, inliers {counts[i]}, stats {st[i]}")
        assert rot < 1.0 and tr < 0.1 and masks[i][sc["true_inlier"]].mean() > 0.95


# ------------------------------------------------------------------------------------------------ batching
def _ragged(rng, B, special, where):
    sizes = [0, 2, 3, 4, 200, 700]
    out = []
    for b in range(B):
        if b == where:
            out.append(special)
            continue
        n = sizes[b % len(sizes)]
        sc = ref.make_scene(rng, max(n, 1), 0.5, 0.3)
        out.append((sc["X"][:n], sc["px"][:n]))
    return out


def test_result_is_bit_identical_alone_and_at_either_end_of_ragged_batches(gpu_ctx, scenes):
    import slamhip

    sc = scenes[1][1]
    special = (sc["X"], sc["px"])
    alone = slamhip.solve_pnp_ransac_batch([special], K, seed=5, refine=False, ctx=gpu_ctx)
    assert alone[3][0, 0] > 100 and alone[3][0, 1] >= 0
    for B in (2, 17, 256):
        for where in (0, B - 1):
            cands = _ragged(np.random.default_rng(100 + B), B, special, where)
            poses, masks, counts, st, _ = slamhip.solve_pnp_ransac_batch(cands, K, seed=5, refine=False, ctx=gpu_ctx)
            assert np.array_equal(poses[where].view(np.uint64), alone[0][0].view(np.uint64)) and np.array_equal(masks[where], alone[1][0]) \
                and np.array_equal(st[where], alone[3][0]), (B, where)
            for b, (Xb, _) in enumerate(cands):
                if len(Xb) < 3:
                    assert np.array_equal(poses[b], np.eye(4)[:3]) and not masks[b].any() and st[b].tolist() == [0, -1, -1, 0]
                else:                                               # (3 or 4 correspondences with an outlier among them may have no model)
                    assert st[b, 0] == masks[b].sum() and (len(Xb) < 200 or (st[b, 0] >= 100 and st[b, 3] > 0))
    again = slamhip.solve_pnp_ransac_batch([special], K, seed=5, refine=False, ctx=gpu_ctx)
    assert _same(again[0], alone[0]) and np.array_equal(again[3], alone[3])            # run to run
    ok, pose1, mask1 = slamhip.solve_pnp_ransac(sc["X"], sc["px"], K, seed=5, refine=False, ctx=gpu_ctx)
    assert ok and np.array_equal(pose1, alone[0][0]) and np.array_equal(mask1, alone[1][0])


def test_a_degenerate_candidate_changes_no_other_candidate(gpu_ctx):
    import slamhip

    rng = np.random.default_rng(11)
    fam = ref.edge_families()
    base = [(s["X"], s["px"]) for s in (ref.make_scene(rng, 50 + (b % 5) * 40, 0.5, 0.3) for b in range(64))]
    empty = (np.zeros((0, 3)), np.zeros((0, 2)))
    for where in (0, 31, 63):
        for name in ("all_nan", "collinear", "huge"):
            a, b = list(base), list(base)
            a[where], b[where] = (fam[name]["X"], fam[name]["px"]), empty
            ra = slamhip.solve_pnp_ransac_batch(a, K, 64, refine=False, ctx=gpu_ctx)
            rb = slamhip.solve_pnp_ransac_batch(b, K, 64, refine=False, ctx=gpu_ctx)
            for k in range(64):
                if k != where:
                    assert np.array_equal(ra[0][k].view(np.uint64), rb[0][k].view(np.uint64)) and np.array_equal(ra[1][k], rb[1][k]) \
                        and np.array_equal(ra[3][k], rb[3][k]), (where, name, k)
            assert np.isfinite(ra[0]).all()


def test_bad_offsets_never_leave_the_arrays_and_are_counted(gpu_ctx):
    import slamhip

    sc = ref.make_scene(np.random.default_rng(32), 300, 0.5, 0.0)
    n = ctypes.c_int64(-1)
    gpu_ctx.lib.slam_index_errors(gpu_ctx.handle, ctypes.byref(n))     # clear
    off = np.array([-50, 100, 10 ** 6, 300], np.int32)                  # starts before 0; leaves the arrays; descends
    pose, mask, st = slamhip.solve_pnp_ransac_offsets(sc["X"], sc["px"], off, K, 64, 8.0, 0, ctx=gpu_ctx)
    assert gpu_ctx.lib.slam_index_errors(gpu_ctx.handle, ctypes.byref(n)) == 0
    assert n.value == 3                                                 # three clamped candidates
    p0, m0, s0 = tw.ransac(sc["X"][:100], sc["px"][:100], K, 64, 8.0, 0)   # candidate 0 shrank to [0, 100)
    p1, m1, s1 = tw.ransac(sc["X"][100:], sc["px"][100:], K, 64, 8.0, 0)   # candidate 1 shrank to [100, 300)
    assert np.array_equal(pose[0], p0) and np.array_equal(mask[:100], m0) and np.array_equal(st[0], s0)
    assert np.array_equal(pose[1], p1) and np.array_equal(mask[100:], m1) and np.array_equal(st[1], s1)
    assert st[2].tolist() == [0, -1, -1, 0] and np.array_equal(pose[2], np.eye(4)[:3])     # candidate 2 shrank to nothing
    pose, mask, st = slamhip.solve_pnp_ransac_offsets(sc["X"], sc["px"], [50, 100, 280], K, 64, 8.0, 0, ctx=gpu_ctx)
    assert not mask[:50].any() and not mask[280:].any()                 # a table that leaves gaps is fine: entries outside are 0
    gpu_ctx.lib.slam_index_errors(gpu_ctx.handle, ctypes.byref(n))
    assert n.value == 0


# ------------------------------------------------------------------------------------------------ the kernel's own boundaries
@pytest.mark.parametrize("n", [3, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 5])
def test_sizes_across_the_lds_chunk(gpu_ctx, n):
    import slamhip

    sc = ref.make_scene(np.random.default_rng(300 + n), n, 0.5, 0.0 if n == 3 else 0.3)
    pose, mask, st = slamhip.solve_pnp_ransac_offsets(sc["X"], sc["px"], [0, n], K, 64, 8.0, 2, ctx=gpu_ctx)
    pt, mt, stt = tw.ransac(sc["X"], sc["px"], K, 64, 8.0, 2)
    assert np.array_equal(pose[0].view(np.uint64), pt.view(np.uint64)) and np.array_equal(mask, mt) and np.array_equal(st[0], stt)
    assert st[0, 0] >= 3


@pytest.mark.parametrize("H", [1, 63, 64, 65, 257])
def test_hypothesis_counts_across_the_wave_and_the_block(gpu_ctx, scenes, H):
    import slamhip

    sc = scenes[2][1]
    pose, mask, st = slamhip.solve_pnp_ransac_offsets(sc["X"], sc["px"], [0, 200], K, H, 8.0, 9, ctx=gpu_ctx)
    pt, mt, stt = tw.ransac(sc["X"], sc["px"], K, H, 8.0, 9)
    assert np.array_equal(pose[0].view(np.uint64), pt.view(np.uint64)) and np.array_equal(mask, mt) and np.array_equal(st[0], stt)
    assert 0 <= st[0, 1] < H


# ------------------------------------------------------------------------------------------------ refinement
def test_refinement_from_the_ransac_pose(gpu_ctx, scenes):
    """Stated relation.  Noise-free scenes (where no outlier happened to vote): the refined pose is no farther from the truth
    than the RANSAC pose (|R - R_true| and |t - t_true|, up to 1e-9 of rounding: both are exact to about 1e-11).  Noisy scenes: the refinement is given the RANSAC inliers and
    ends by classifying them at chi2 <= 5.991^2 under ITS pose; an edge it drops has chi2 above the gate there, so
    refined count = RANSAC count - #{RANSAC inliers with chi2 above the gate at the refined pose}, asserted as
    'at least' against that number recomputed in numpy (an edge within 1e-9 of the gate may fall either way)."""
    import slamhip
    from slamhip.pose_opt import CHI2_THRESHOLD

    rng = np.random.default_rng(77)
    clean = [ref.make_scene(rng, 200, 0.0, share) for share in (0.0, 0.3, 0.5)]
    allsc = clean + [sc for _, sc in scenes]
    cands = [(sc["X"], sc["px"]) for sc in allsc] + [(np.zeros((2, 3)), np.zeros((2, 2)))]
    raw = slamhip.solve_pnp_ransac_batch(cands, K, refine=False, ctx=gpu_ctx)
    fin = slamhip.solve_pnp_ransac_batch(cands, K, refine=True, ctx=gpu_ctx)
    assert raw[4] is None and fin[4].shape == (len(cands),)
    assert all(np.array_equal(a, b) for a, b in zip(raw[1], fin[1])) and np.array_equal(raw[3], fin[3])      # the mask stays the RANSAC vote
    assert np.array_equal(fin[0][-1], np.eye(4)[:3]) and fin[4][-1] == 0 and fin[3][-1].tolist() == [0, -1, -1, 0]   # no model: not refined
    for i, sc in enumerate(allsc):
        r0, t0 = ref.pose_errors(raw[0][i], sc)
        r1, t1 = ref.pose_errors(fin[0][i], sc)
        m = raw[1][i]
        Y = sc["X"][m] @ fin[0][i][:, :3].T + fin[0][i][:, 3]
        e = np.stack([K[0] * Y[:, 0] / Y[:, 2] + K[2], K[1] * Y[:, 1] / Y[:, 2] + K[3]], 1) - sc["px"][m]
        chi2 = (e * e).sum(1)
        above = int((chi2 > CHI2_THRESHOLD * (1 - 1e-9)).sum())
        print(f"scene {i}: ransac rot {r0:.2e} dt {t0:.2e} -> refined rot {r1:.2e} dt {t1:.2e}; inliers {raw[2][i]} -> {fin[4][i]} (above the gate {above})")
        assert fin[4][i] >= raw[2][i] - above and fin[4][i] <= raw[2][i]
        if i < len(clean):
            if not m[~sc["true_inlier"]].any():
                d0, d1 = np.linalg.norm(raw[0][i][:, :3] - sc["R"]), np.linalg.norm(fin[0][i][:, :3] - sc["R"])
                print(f"         |dR| {d0:.2e} -> {d1:.2e}")
                assert d1 <= d0 + 1e-9 and t1 <= t0 + 1e-9
        else:
            assert r1 < 1.0 and t1 < 0.1


def test_backend_relocalize_and_loop_edges(gpu_ctx, scenes):
    import slamhip
    from backend import Backend

    cands = [(sc["X"], sc["px"]) for _, sc in scenes[:3]]
    poses, counts, masks = Backend().relocalize(cands, *K)
    fin = slamhip.solve_pnp_ransac_batch(cands, K, ctx=gpu_ctx)
    assert poses.shape == (3, 4, 4) and np.array_equal(poses[:, :3], fin[0]) and np.array_equal(counts, fin[2])
    Tm = np.tile(np.eye(4), (4, 1, 1))
    edges, meas, info = slamhip.loop_edges_from_pnp([[0, 1], [0, 2], [0, 3]], poses, counts, Tm)
    assert len(edges) == 3 and np.abs(meas - poses[:, :3]).max() < 1e-15 and (np.diagonal(info, axis1=1, axis2=2) > 0).all()


# ------------------------------------------------------------------------------------------------ the batch amortises the launch
def test_a_batch_of_256_candidates_takes_less_than_256_single_calls(gpu_ctx):
    rng = np.random.default_rng(70)
    sc = [ref.make_scene(rng, 200, 0.5, 0.3) for _ in range(256)]
    X = np.concatenate([s["X"] for s in sc])
    px = np.concatenate([s["px"] for s in sc])
    off = np.arange(257, dtype=np.int32) * 200
    dX, dp, do = gpu_ctx.upload(X), gpu_ctx.upload(px), gpu_ctx.upload(off)
    dT, dm, ds = gpu_ctx.malloc(256 * 96), gpu_ctx.malloc(len(X)), gpu_ctx.malloc(256 * 16)
    lib, h = gpu_ctx.lib, gpu_ctx.handle

    def batch():
        assert lib.slam_pnp_ransac_f64(h, 256, do.ptr, dX.ptr, dp.ptr, len(X), *K, 256, 8.0, 0, dT.ptr, dm.ptr, ds.ptr) == 0

    def singles():
        for b in range(256):
            assert lib.slam_pnp_ransac_f64(h, 1, do.ptr + 4 * b, dX.ptr, dp.ptr, len(X), *K, 256, 8.0, 0, dT.ptr + 96 * b, dm.ptr,
                                           ds.ptr + 16 * b) == 0

    def timed(fn):
        gpu_ctx.timer_start()
        fn()
        return gpu_ctx.timer_stop()

    try:
        timed(batch), timed(singles)                      # warm-up
        tb = np.median([timed(batch) for _ in range(5)])
        Tb = dT.download(np.float64, (256, 12))
        ts = np.median([timed(singles) for _ in range(5)])
        print(f"256 candidates x 200 correspondences, H = 256: batch {tb:.3f} ms, 256 single calls {ts:.3f} ms")
        assert np.array_equal(dT.download(np.float64, (256, 12)), Tb)
        assert tb < ts
    finally:
        for o in (dX, dp, do, dT, dm, ds):
            o.free()
