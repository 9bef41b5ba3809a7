"""The covisibility graph on the device (csrc/covis.hip) against slamhip.covisibility and the brute-force statement of
tests/covis_ref.py, bit for bit; its refusals; and the sparse bundle adjustment on its tables against the host's."""
import numpy as np
import pytest

import ba_sparse_cases as BC
import ba_sparse_ref as R
import covis_cases as C
from covis_ref import covisibility_ref, same_tables

pytestmark = pytest.mark.gpu


class Allocations:
    """Every buffer the context hands out while this is installed; ``live`` are the ones not freed yet."""

    def __init__(self, ctx, monkeypatch):
        self.buffers = []
        malloc = ctx.malloc

        def tracked(nbytes):
            self.buffers.append(malloc(nbytes))
            return self.buffers[-1]

        monkeypatch.setattr(ctx, "malloc", tracked, raising=False)

    @property
    def live(self):
        return [b for b in self.buffers if b.ptr]


def _device(ctx, case, **kw):
    from slamhip import covisibility_device

    K, L, op, ol, fixed = case
    tab = covisibility_device(op, ol, K, fixed, L, ctx=ctx, **kw)
    try:
        out = tab.download()
        assert (tab.E, tab.P) == (len(out[0]), len(out[3])) and np.array_equal(tab.edges, out[0]) and np.array_equal(tab.weights, out[1])
        return out
    finally:
        tab.free()


@pytest.mark.parametrize("name", C.names(masked=True))
def test_device_equals_host_function(gpu_ctx, name):
    from slamhip import covisibility

    K, L, op, ol, fixed = C.cases()[name]
    assert same_tables(_device(gpu_ctx, C.cases()[name]), covisibility(op, ol, K, fixed, L))


@pytest.mark.parametrize("name", C.names(masked=False))
def test_device_equals_reference_without_a_mask(gpu_ctx, name):
    K, L, op, ol, fixed = C.cases()[name]
    assert fixed is None
    assert same_tables(_device(gpu_ctx, C.cases()[name]), covisibility_ref(op, ol, K))


def test_number_of_points_left_to_the_call(gpu_ctx):
    from slamhip import covisibility, covisibility_device

    K, L, op, ol, fixed = C.cases()["gaps"]
    tab = covisibility_device(op, ol, K, fixed, ctx=gpu_ctx)
    try:
        assert tab.L == int(ol.max()) + 1 < L and same_tables(tab.download(), covisibility(op, ol, K, fixed))
        assert tab.free_observations == int((~fixed[op]).sum())
    finally:
        tab.free()


def test_order_of_the_observation_list(gpu_ctx):
    from slamhip import covisibility

    base = C.cases()["fixed-in-the-middle"]
    first = None
    for seed in (1, 2, 3):
        case, perm = C.permuted(base, seed)
        got = _device(gpu_ctx, case)
        assert same_tables(got, covisibility(case[2], case[3], case[0], case[4], case[1]))
        named = got[:3] + (perm[got[3]], perm[got[4]])            # the pairs as observations of the unpermuted list
        if first is None:
            first = named
        assert all(np.array_equal(a, b) for a, b in zip(named, first))
    again = [_device(gpu_ctx, C.cases()["configs4-scaled"]) for _ in range(2)]
    assert all(a.tobytes() == b.tobytes() for a, b in zip(*again))


def test_from_observations(gpu_ctx):
    from slamhip import CovisibilityTables, MapObservations

    K, lists = C.map_observations()
    mo = MapObservations.from_lists(lists, gpu_ctx)
    slot_pose = mo.obs[:, 0]
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
            assert (slot_pose[got[3]] == np.repeat(got[0][:, 0], got[1])).all() and (slot_point[got[3]] == slot_point[got[4]]).all()
        with pytest.raises(ValueError, match="out of range"):
            CovisibilityTables.from_observations(mo, K - 1)
        with pytest.raises(ValueError, match="fixed pose"):
            CovisibilityTables.from_observations(mo, K, np.zeros(K, bool))
        empty = MapObservations.from_lists([[], []], gpu_ctx)
        try:
            tab = CovisibilityTables.from_observations(empty, 4)
            assert (tab.E, tab.P) == (0, 0) and tab.download()[2].tolist() == [0]
            tab.free()
        finally:
            empty.free()
    finally:
        mo.free()


def test_refusals_leave_nothing_behind(gpu_ctx, monkeypatch):
    from slamhip import covisibility, covisibility_device

    base = C.refusal_base()
    K, L, op, ol, fixed = base
    assert len(op) > 10 ** 4 + 10
    want = covisibility(op, ol, K, fixed, L)
    on_fixed = int(np.flatnonzero(fixed[op])[0])
    E, P = len(want[0]), len(want[3])
    refused = [("adjacent", C.with_duplicate(base, 100, 1), {}, "observed more than once"),
               ("far apart", C.with_duplicate(base, 17, 10 ** 4), {}, "observed more than once"),
               ("on a fixed pose", C.with_duplicate(base, on_fixed, 5000), {}, "observed more than once"),
               ("pose out of range", (K, L, np.r_[op, K].astype(np.int32), np.r_[ol, 0].astype(np.int32), fixed), {}, "out of range"),
               ("negative point", (K, L, op, np.r_[-1, ol[1:]].astype(np.int32), fixed), {}, "out of range"),
               ("point past L", (K, L, op, np.r_[L, ol[1:]].astype(np.int32), fixed), {}, "out of range"),
               ("no fixed pose", (K, L, op, ol, np.zeros(K, bool)), {}, "at least one fixed pose"),
               ("pair limit", base, dict(_limits=(P - 1, E)), f"{P} covisible pairs: more than the {P - 1}"),
               ("edge limit", base, dict(_limits=(P, E - 1)), f"{E} covisibility edges: more than the {E - 1}")]
    alloc = Allocations(gpu_ctx, monkeypatch)
    for what, case, kw, message in refused:
        for fn in (covisibility, None):                           # the host function refuses the same input with the same words
            if fn is not None and kw:
                continue
            with pytest.raises(ValueError, match=message):
                if fn is not None:
                    fn(case[2], case[3], case[0], case[4], case[1])
                else:
                    covisibility_device(case[2], case[3], case[0], case[4], case[1], ctx=gpu_ctx, **kw)
        assert not alloc.live, what
        assert same_tables(_device(gpu_ctx, base, _limits=(P, E)), want), what          # the context still serves, at the limits too
        assert not alloc.live, what
    assert len(alloc.buffers) > 9 * 8


def _window_problem(ctx, w, mode):
    from slamhip import SparseBAProblem

    K, L = len(w["T0"]), len(w["X0"])
    fixed = np.zeros(K, bool)
    fixed[list(w["fixed"])] = True
    prob = SparseBAProblem(ctx, K, L, w["op"], w["ol"], w["meas"], R.INTR, fixed, covisibility=mode)
    prob.set_state(w["T0"][:, :3, :4].reshape(K, 12), w["X0"])
    return prob


_windows = {}


def _window(name):
    if name not in _windows:
        _windows[name] = BC.random_window(BC.hub_layout()) if name == "hub41" else R.case_edges()
    return _windows[name]


@pytest.mark.parametrize("name", ["hub41", "fixed-in-the-middle"])
def test_sparse_ba_on_device_tables_equals_host_tables(gpu_ctx, monkeypatch, name):
    from slamhip import bundle_adjust_sparse

    w = _window(name)
    if name == "fixed-in-the-middle":
        assert 0 < min(w["fixed"][1:]) and max(w["fixed"]) < len(w["T0"]) - 1
    alloc = Allocations(gpu_ctx, monkeypatch)
    systems = {}
    for mode in ("host", "device"):
        prob = _window_problem(gpu_ctx, w, mode)
        try:
            prob.linearize(1.0)
            prob.reduce(0.125)
            systems[mode] = prob.reduced_system() + (prob.edges, prob.weights, prob.d_pair_ptr.download(np.int32, (prob.E + 1,)),
                                                     prob.d_pair_a.download(np.int32, (prob.P,)), prob.d_pair_b.download(np.int32, (prob.P,)))
            assert prob.E > 0 and prob.P >= prob.E
        finally:
            prob.free()
        assert not alloc.live
    assert all(a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes() for a, b in zip(systems["host"], systems["device"]))
    runs = {}
    for mode in ("host", "device"):
        runs[mode] = bundle_adjust_sparse(w["T0"], w["X0"], w["op"], w["ol"], w["meas"], R.INTR, iterations=4, fixed_poses=w["fixed"],
                                          huber_delta=1.0, ctx=gpu_ctx, covisibility=mode)
        assert not alloc.live
    (a, sa), (b, sb) = runs["host"], runs["device"]
    assert a.poses.tobytes() == b.poses.tobytes() and a.points.tobytes() == b.points.tobytes() and sa == sb
    assert (a.chi2_initial, a.chi2_final, a.iterations) == (b.chi2_initial, b.chi2_final, b.iterations) and a.iterations > 0


def test_sparse_ba_refusals_with_device_tables(gpu_ctx, monkeypatch):
    from slamhip import bundle_adjust_sparse

    w = _window("hub41")
    alloc = Allocations(gpu_ctx, monkeypatch)
    args = lambda op, ol, meas: (w["T0"], w["X0"], op, ol, meas, R.INTR)
    with pytest.raises(ValueError, match="observed more than once"):
        bundle_adjust_sparse(*args(np.r_[w["op"], w["op"][3]], np.r_[w["ol"], w["ol"][3]], np.r_[w["meas"], w["meas"][3:4]]), fixed_poses=w["fixed"],
                             ctx=gpu_ctx, covisibility="device")
    with pytest.raises(ValueError, match="'host' or 'device'"):
        bundle_adjust_sparse(*args(w["op"], w["ol"], w["meas"]), fixed_poses=w["fixed"], ctx=gpu_ctx, covisibility="gpu")
    assert not alloc.live


def test_backend_global_bundle_adjust_with_device_tables(gpu_ctx):
    from backend import Backend

    w = _window("hub41")
    be = Backend()
    run = lambda **kw: be.global_bundle_adjust(w["T0"], w["X0"], w["op"], w["ol"], w["meas"], *R.INTR, iterations=4, fixed_poses=w["fixed"],
                                               huber_delta=1.0, **kw)
    (a, sa), (b, sb) = run(), run(covisibility="device")
    assert a.poses.tobytes() == b.poses.tobytes() and a.points.tobytes() == b.points.tobytes() and sa == sb and sb["pairs"] > 0


def test_backend_covisibility_graph(gpu_ctx):
    from backend import Backend

    K, L, op, ol, fixed = C.cases()["configs4-scaled-nomask"]
    g = Backend().covisibility_graph(op, ol, K)
    edges, weights = covisibility_ref(op, ol, K)[:2]
    assert np.array_equal(g.edges, edges) and np.array_equal(g.weights, weights) and g.K == K
    assert len(g.best(3, 10)) == 10 and g.connected(3).tolist() == [k for k in range(K) if k != 3]


def test_backend_essential_graph_feeds_the_optimiser(gpu_ctx):
    from backend import Backend

    K = 30                                                        # a ring: point l is seen by keyframes l, l + 1, l + 2 (mod 30), ten points each
    tracks = [tuple(sorted((l % K, (l + 1) % K, (l + 2) % K))) for l in range(10 * K)]
    _, _, op, ol, _ = C.from_tracks(K, tracks, None, 77)
    be = Backend()
    g = be.covisibility_graph(op, ol, K)
    assert len(g.edges) == 2 * K and sorted(set(g.weights.tolist())) == [10, 20]
    edges = be.essential_graph_edges(op, ol, K, min_weight=20, loop_edges=[(29, 0), (14, 3)])
    ring = sorted((min(k, (k + 1) % K), max(k, (k + 1) % K)) for k in range(K))
    # the tree (k - 1 is k's heaviest lower neighbour; 1 hangs on 0), the 30 edges of weight 20, and the loop edge (3, 14)
    assert [tuple(e) for e in edges.tolist()] == sorted(set(ring) | {(3, 14)})
    assert np.array_equal(edges, g.essential_edges(20, [(29, 0), (14, 3)])) and np.array_equal(be.essential_graph_edges(op, ol, K, 20), np.array(ring))
    ang = 2 * np.pi * np.arange(K) / K
    t = np.stack([4 * np.cos(ang), 4 * np.sin(ang), 0 * ang], 1)
    sims = (np.ones(K), np.tile(np.eye(3), (K, 1, 1)), t + np.random.default_rng(5).normal(0, 0.01, (K, 3)))
    E = len(edges)
    meas = (np.ones(E), np.tile(np.eye(3), (E, 1, 1)), t[edges[:, 1]] - t[edges[:, 0]])      # S_j S_i^-1 of pure translations
    (s, Rm, tt), st = be.optimize_essential_graph(sims, edges, meas, np.tile(np.eye(7), (E, 1, 1)), fixed=(0,), iterations=5)
    assert np.isfinite(s).all() and np.isfinite(Rm).all() and np.isfinite(tt).all() and st["chi2_final"] < 1e-3 * st["chi2_initial"]
