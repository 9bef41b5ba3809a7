"""The vote block the four batched RANSAC calls share (csrc/geometry_host.h) on the device: a call that follows a larger one on
the same context reads no stale key and no stale model count, and its grid covers its hypotheses.

On one context a call of B = 3 candidates of 8 correspondences each with H = 257 comes first; the call under test has B = 2,
a first candidate one correspondence short of the minimal sample and a second of 8, and runs with H = 1 and H = 257 (one
hypothesis past a block of 256), the two-view call, whose blocks hold 64 hypotheses, with H = 65 as well.  Model, mask and
stats of the second call are the host twin's, bit for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = 11


def _family(name):
    """(correspondence arrays a, b of 24 rows, the minimal sample, run(ctx, cands, H) -> (models [B,w], masks, stats), twin(x, y, H))"""
    import slamhip

    if name == "two_view":
        import two_view_ref as ref
        from oracle import oracle
        sc = ref.make_scene(np.random.default_rng(9301), 24, 0.5, 0.3)

        def run(ctx, cands, H):
            E, masks, st = slamhip.find_essential_batch(cands, ref.EUROC, H, 1.0, SEED, ctx=ctx)
            return E.reshape(-1, 9), masks, st
        return sc["px1"], sc["px2"], 5, run, lambda x, y, H: oracle.tv_twin_ransac(x, y, ref.EUROC, H, 1.0, SEED)
    if name == "homography":
        import hg_twin as tw
        import homography_ref as hr
        sc = hr.scenes_planar_noisy(seed=4, n=24)[1]

        def run(ctx, cands, H):
            Hm, masks, st = slamhip.find_homography_batch(cands, H, 3.0, SEED, ctx=ctx)
            return Hm.reshape(-1, 9), masks, st
        return sc["px1"], sc["px2"], 4, run, lambda x, y, H: tw.ransac(x, y, H, 3.0, SEED)
    if name == "pnp":
        import pnp_ref as ref
        import pnp_twin as tw
        sc = ref.make_scene(np.random.default_rng(9303), 24, 0.5, 0.3)

        def run(ctx, cands, H):
            poses, masks, _counts, st, _ = slamhip.solve_pnp_ransac_batch(cands, ref.EUROC, H, 8.0, SEED, refine=False, ctx=ctx)
            return poses.reshape(-1, 12), masks, st
        return sc["X"], sc["px"], 3, run, lambda x, y, H: tw.ransac(x, y, ref.EUROC, H, 8.0, SEED)
    import sim3_ref as ref
    import sim3_twin as tw
    sc = ref.make_scene(np.random.default_rng(9304), 24, 1.3, 0.001, 0.3)

    def run(ctx, cands, H):
        s, R, t, masks, st, _ = slamhip.estimate_sim3_batch(cands, ref.EUROC, H, ref.CHI2, False, SEED, refit=False, ctx=ctx)
        return np.stack([ref.pack(s[i], R[i], t[i]) for i in range(len(s))]), masks, st
    return sc["X1"], sc["X2"], 3, run, lambda x, y, H: tw.ransac(x, y, ref.EUROC, H, ref.CHI2, SEED)


CASES = [(f, H) for f in ("two_view", "homography", "pnp", "sim3") for H in ((1, 65, 257) if f == "two_view" else (1, 257))]


@pytest.mark.parametrize("family,H", CASES)
def test_a_smaller_call_after_a_larger_one_is_the_twins(built, family, H):
    import slamhip

    a, b, minimal, run, twin = _family(family)
    larger = [(a[8 * i:8 * i + 8], b[8 * i:8 * i + 8]) for i in range(3)]
    short = minimal - 1
    cands = [(a[:short], b[:short]), (a[8:16], b[8:16])]
    want = [twin(x, y, H) for x, y in cands]
    ctx = slamhip.Context()
    try:
        first = run(ctx, larger, 257)
        assert first[2][:, 3].max() > 0                               # the larger call scored models: its keys and counts are not zero
        models, masks, st = run(ctx, cands, H)
    finally:
        ctx.close()
    assert st[0].tolist() == [0, -1, -1, 0] and len(masks[0]) == short and not masks[0].any()      # below the minimal sample: "no model"
    for i, (m, mask, s) in enumerate(want):
        assert np.ascontiguousarray(models[i], np.float64).tobytes() == np.ascontiguousarray(m, np.float64).reshape(-1).tobytes(), (i, models[i], m)
        assert np.array_equal(np.asarray(masks[i], np.uint8), np.asarray(mask, np.uint8).reshape(-1)), i
        assert st[i].tolist() == np.asarray(s).tolist(), (i, st[i], s)
