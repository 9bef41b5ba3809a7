"""The covisibility graph on the device (csrc/covis.hip) in the forms tests/test_covis_gpu.py never selects, bit for bit
(tests/covis_edge_cases.py; the cases' premises are asserted by tests/test_covis_edges_cpu.py): observation keys of 31, 32 and
33 bits and of 46, with entries out of range; 64-bit pair keys over one to three sort tiles in five and six passes; a list of
2 896 poses and head and pair scans three levels deep; ``cv_rows`` on 200 000 points.  Every case runs with its mask and in
graph mode.  The small cases are held to slamhip.covisibility and to the brute force, the ones of millions of pairs to tables
stated in closed form from their construction."""
import ctypes

import numpy as np
import pytest

import covis_cases as C
import covis_edge_cases as X
from covis_ref import covisibility_ref, same_tables
from test_covis_gpu import Allocations, _device

pytestmark = pytest.mark.gpu

WIDE = [n for n, v in X.width_sizes().items() if v[2] >= 32]          # the 32-bit key with its top bit in use, and every 64-bit one


def _index_errors(ctx):
    """The count since the last call (reading resets it)."""
    n = ctypes.c_int64(0)
    assert ctx.lib.slam_index_errors(ctx.handle, ctypes.byref(n)) == 0
    return n.value


def _both_modes(ctx, name, case):
    from slamhip import covisibility

    K, L, op, ol, fixed = case
    assert same_tables(_device(ctx, case), covisibility(op, ol, K, fixed, L))
    assert same_tables(_device(ctx, X.masked(case, False)), X.expected(name, case, False))


# ---- 1. the width of the observation key ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(X.width_sizes()))
def test_observation_keys_of_31_to_46_bits(gpu_ctx, name):
    _both_modes(gpu_ctx, name, X.width_case(name))


@pytest.mark.parametrize("name", WIDE)
def test_entries_out_of_range_are_counted_and_refused(gpu_ctx, monkeypatch, name):
    """Through the count phase and ``build_tables`` on device arrays (``covisibility_device`` refuses such a list on the
    host): the key of an entry out of range is L << (pb + 1), in 32 bits with the top bit set, in 33 the only key with bit 32."""
    from slamhip import covis, covisibility_device

    ctx, base = gpu_ctx, X.width_case(name)
    (K, L, op, ol, fixed), n_bad = X.with_bad_entries(base, 9)
    alloc = Allocations(ctx, monkeypatch)
    with pytest.raises(ValueError, match="out of range"):
        covisibility_device(op, ol, K, fixed, L, ctx=ctx)
    assert not alloc.buffers
    _index_errors(ctx)
    for on in (True, False):
        want = X.expected(name, base, on)
        held = []
        try:
            d_op, d_ol = covis._up(ctx, held, op), covis._up(ctx, held, ol)
            d_fx = covis._up(ctx, held, fixed.astype(np.uint8)) if on else None
            ws = covis._new(ctx, held, covis.workspace_bytes(K, L, len(op))[0])
            s = (ctypes.c_int64 * 4)()
            covis.check(ctx.lib.slam_covis_count(ctx.handle, K, L, len(op), d_op.ptr, d_ol.ptr, d_fx.ptr if on else None, ws.ptr, s))
            # free observations, duplicates, P: those of the list without the bad entries, which lie behind every point
            assert list(s) == [int((~fixed[base[2]]).sum()) if on else len(base[2]), 0, len(want[3]), n_bad]
            assert _index_errors(ctx) == n_bad
            with pytest.raises(ValueError, match="out of range"):
                covis.build_tables(ctx, d_op, d_ol, d_fx, K, L, len(op))
            assert _index_errors(ctx) == n_bad
        finally:
            for b in held:
                b.free()
        assert not alloc.live
        assert same_tables(_device(ctx, X.masked(base, on)), want) and not alloc.live        # the context still serves
    assert _index_errors(ctx) == 0


# ---- 2. 64-bit pair keys over more than one sort tile ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(X.pair_key_sizes()))
def test_pair_keys_of_64_bits_over_sort_tiles(gpu_ctx, name):
    _both_modes(gpu_ctx, ("pairkeys", name), X.pair_key_case(name)[0])


# ---- 3. scans three levels deep ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", range(len(X.hub_pairs_sizes())))
def test_hub_of_thousands_and_head_ranks_three_levels_deep(gpu_ctx, which):
    """P = S - 1, S, S + 1 and S + scan_tile + 1 pairs (S = scan_tile^2: two, two, three and three levels of the scan that
    ranks the run heads), 4 191 960 of them from one list of 2 896 poses, against the closed form of covis_edge_cases.hub_case."""
    n, P = X.hub_size(), X.hub_pairs_sizes()[which]
    case, want = X.hub_case(n, P - n * (n - 1) // 2, 70 + which)
    K, L, op, ol, fixed = case
    h = int(np.bincount(ol).argmax())
    at = np.zeros(K, np.int64)
    at[op[ol == h]] = np.flatnonzero(ol == h)                          # where pose k's observation of the hub is
    row_start = lambda i: i * (2 * n - i - 1) // 2                     # noqa: E731
    assert len(want[3]) == P and (ol == h).sum() == n
    for on in (True, False):
        edges, weights, ptr, pa, pb = got = _device(gpu_ctx, X.masked(case, on))
        assert same_tables(got, want)
        # the first and the last slot of rows 0, 1, n - 3 and n - 2 of the triangle (so the first and the last pair of the
        # hub), from the row starts alone
        for i in (0, 1, n - 3, n - 2):
            for e, k1, k2 in ((row_start(i), i + 1, i + 2), (row_start(i + 1) - 1, i + 1, n)):
                a, b = pa[ptr[e]:ptr[e + 1]], pb[ptr[e]:ptr[e + 1]]
                assert edges[e].tolist() == [k1, k2] and (op[a] == k1).all() and (op[b] == k2).all()
                assert (ol[a] == ol[b]).all() and (np.diff(ol[a]) > 0).all() and weights[e] == len(a)
                assert a[ol[a] == h].tolist() == [at[k1]] and b[ol[b] == h].tolist() == [at[k2]]
        assert edges[-1].tolist() == [n - 1, n] and (ptr[-2], ptr[-1], weights[-1]) == (P - 1, P, 1) and len(edges) == n * (n - 1) // 2


@pytest.mark.parametrize("which", range(len(X.points_sizes())))
def test_pair_scan_over_points_three_levels_deep(gpu_ctx, which):
    """L + 1 = S, S + 1 and S + scan_tile + 3 entries of the 64-bit pair scan: two, three and three levels."""
    L = X.points_sizes()[which]
    _both_modes(gpu_ctx, ("points", L), X.points_case(L))


# ---- 4. cv_rows on a large map -------------------------------------------------------------------------------------------------------
def test_from_observations_of_a_large_map(gpu_ctx):
    from slamhip import CovisibilityTables, MapObservations

    K, offsets, obs = X.large_map()
    mo = MapObservations.from_arrays(offsets, obs, gpu_ctx)
    slot_pose = obs[:, 0]
    slot_point = np.repeat(np.arange(len(mo)), mo.nobs).astype(np.int32)
    fixed = np.zeros(K, bool)
    fixed[[0, 31]] = True
    try:
        for mask in (None, fixed):
            tab = CovisibilityTables.from_observations(mo, K, mask)
            try:
                got = tab.download()
            finally:
                tab.free()
            assert same_tables(got, covisibility_ref(slot_pose, slot_point, K, mask))
            if mask is None:                                          # the first and the last observed point both have pairs
                assert slot_point[got[3]].min() == X.MAP_EMPTY_ENDS and slot_point[got[3]].max() == X.MAP_POINTS - X.MAP_EMPTY_ENDS - 1
    finally:
        mo.free()


# ---- 5. order and repeat -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group, name", [("width", "K65537-L16384"), ("pairkeys", f"K{1 << 24}-P{2 * X.limits()['sort_tile'] + 1}")])
def test_order_of_the_observation_list_and_two_runs(gpu_ctx, group, name):
    base = X.width_case(name) if group == "width" else X.pair_key_case(name)[0]
    want = X.expected(name if group == "width" else (group, name), base, True)
    runs = {}
    for seed in (1, 2, 1):
        case, perm = C.permuted(base, seed)
        got = _device(gpu_ctx, case)
        named = got[:3] + (perm[got[3]], perm[got[4]])                # the pairs as observations of the unpermuted list
        assert all(np.array_equal(a, b) for a, b in zip(named, want))
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, runs.setdefault(seed, got)))      # two runs: equal bytes
