"""GPU: the kernels of csrc/ba_sparse.hip phase by phase on exactly-stated problems (tests/ba_sparse_cases.py; the premises
are asserted by tests/test_ba_sparse_edges_cpu.py).

EXACT tests compare bytes, with no tolerance (`C.same_bits`; only the sign of a zero is dropped): the linearisation on grid
scenes (every term a dyadic rational of few bits, so the f64 sums are the exact ones in any order), and reduce,
back-substitution and candidate on integer blocks with unimodular point blocks.  BOUNDED tests (the random scene) take their
bound from the terms alone - (terms + CHAIN_ROUNDINGS) * 2^-52 * sum of |terms|, no condition number - twice, because two
evaluations are compared; each prints the worst ratio it met.  The guard tests go through the raw entry points with every
table inside a larger allocation of bait, and send no index that the kernels as read would dereference."""
import ctypes
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ba_sparse_cases as C  # noqa: E402
import ba_sparse_ref as R  # noqa: E402
from oracle import oracle  # noqa: E402
from test_ba_limits_gpu import _holds  # noqa: E402

pytestmark = pytest.mark.gpu
_cache = {}


def _once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _rt(T):
    return T[:, :3, :4].reshape(len(T), 12)


def _index_errors(ctx):
    """The count since the last call (reading resets it)."""
    n = ctypes.c_int64(0)
    assert ctx.lib.slam_index_errors(ctx.handle, ctypes.byref(n)) == 0
    return n.value


def _f64bits(x):
    return struct.pack("<d", float(x))


def _worst(diff, bound):
    diff, bound = np.abs(diff), np.broadcast_to(bound, np.shape(diff))
    zero = bound == 0
    assert (diff[zero] == 0).all()
    return float((diff[~zero] / bound[~zero]).max(initial=0.0))


def _problem(ctx, sc):
    from slamhip import SparseBAProblem

    prob = SparseBAProblem(ctx, sc["K"], sc["L"], sc["op"], sc["ol"], sc["meas"], sc["intr"], sc["fixed"])
    prob.set_state(sc["T12"], sc["X"])
    return prob


def _window_problem(ctx, w):
    from slamhip import SparseBAProblem

    K = len(w["T0"])
    fixed = np.zeros(K, bool)
    fixed[list(w["fixed"])] = True
    prob = SparseBAProblem(ctx, K, len(w["X0"]), w["op"], w["ol"], w["meas"], R.INTR, fixed)
    prob.set_state(_rt(w["T0"]), w["X0"])
    return prob


def _lin_blocks(prob):
    K, L, O = prob.K, prob.L, prob.O
    d = lambda b, shape: b.download(np.float64, shape)
    return dict(Hpl=d(prob.d_Hpl, (O, 18)), Hll=d(prob.d_Hll, (L, 6)), bl=d(prob.d_bl, (L, 3)), Hpp=d(prob.d_Hpp, (K, 21)), bp=d(prob.d_bp, (K, 6)),
                cost=d(prob.d_cost, (K,)))


# ---- case 2: the linearisation, exact ------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(6), ids=["long-delta0", "long-delta5", "long-e8-delta5", "long-delta-sqrt2", "k300-pose299", "k300-point299"])
def test_linearize_on_grid_scenes_is_exact(gpu_ctx, i):
    """Every output of slam_bas_linearize_f64 equals the Fraction statement byte for byte: Hpl, Hll, bl, Hpp (packed 21), bp,
    the per-pose cost (poses of 1, 255, 256, 257, 512, 513, 1025 and 1468 observations: up to six trips of the 256-thread
    loop); the total cost is the exact integer; the returned largest diagonal is the maximum over the downloaded free-pose
    Hpp and all Hll, byte for byte, and smaller than the fixed pose's (long layout), or lies at pose / point 299 (K = 300:
    the second trip of the maximum's loop).  delta = sqrt(2) with residuals of norm^2 = 2: the f64 norm EQUALS delta, the
    strict gate keeps rho = 2 where `>=` would give 2 delta en - delta^2, one ulp away."""
    sc, delta = C.grid_scenes()[i]
    ex = C.linearize_exact(sc, delta)
    prob = _problem(gpu_ctx, sc)
    try:
        cost, dmax = prob.linearize(delta)
        got = _lin_blocks(prob)
    finally:
        prob.free()
    for name in ("Hpl", "Hll", "bl", "Hpp", "bp", "cost"):
        assert C.same_bits(got[name], ex[name]), (name, int((got[name] != ex[name]).sum()))
    assert ex["total"].denominator == 1 and _f64bits(cost) == _f64bits(int(ex["total"]))
    free = ~sc["fixed"]
    dg, dg3 = [C.TRI.index((a, a)) for a in range(6)], [C.TRI3.index((a, a)) for a in range(3)]
    assert _f64bits(dmax) == _f64bits(max(got["Hpp"][free][:, dg].max(), got["Hll"][:, dg3].max())) == _f64bits(ex["dmax"])
    if sc["K"] < 100:
        assert got["Hpp"][0][dg].max() > dmax                          # the fixed pose would have won
    elif i == 4:
        assert dmax == got["Hpp"][299][dg].max()
    else:
        assert dmax == got["Hll"][299][dg3].max()


# ---- case 3: the linearisation on the random scene -------------------------------------------------------------------------
@pytest.mark.parametrize("delta", [0.0, 1.0])
def test_linearize_on_the_long_layout_against_numpy(gpu_ctx, delta):
    """Hpl, Hll, bl, Hpp, bp and the per-pose cost on ba_sparse_ref's random scene, each against ba_sparse_ref.linearize
    within twice (terms + CHAIN_ROUNDINGS) * 2^-52 * sum of |terms|, the terms being the summands (cases.linearize_bound).
    Met to 0.05 of the bound on the MI355X (profiles/ba_sparse_edges_gpu_tests.log)."""
    w = _once("long-window", lambda: C.random_window(C.long_layout()))
    ref = R.linearize(_rt(w["T0"]), w["X0"], w["op"], w["ol"], w["meas"], R.INTR, delta)
    bound = C.linearize_bound(_rt(w["T0"]), w["X0"], w["op"], w["ol"], w["meas"], R.INTR, delta)
    prob = _window_problem(gpu_ctx, w)
    try:
        cost, _ = prob.linearize(delta)
        got = _lin_blocks(prob)
    finally:
        prob.free()
    K, L, O = len(w["T0"]), len(w["X0"]), len(w["op"])
    full = lambda packed, tri, n: np.stack([packed[:, tri.index((min(a, c), max(a, c)))] for a in range(n) for c in range(n)], 1).reshape(-1, n, n)
    ratios = dict(Hpl=_worst(got["Hpl"].reshape(O, 6, 3) - ref["Hpl"], bound["Hpl"]), Hll=_worst(full(got["Hll"], C.TRI3, 3) - ref["Hll"], bound["Hll"]),
                  bl=_worst(got["bl"] - ref["bl"], bound["bl"]), Hpp=_worst(full(got["Hpp"], C.TRI, 6) - ref["Hpp"], bound["Hpp"]),
                  bp=_worst(got["bp"] - ref["bp"], bound["bp"]), cost=_worst(got["cost"] - ref["cost_pose"], bound["cost"]))
    print(f"\nlinearise, long layout, delta={delta}: |difference| / bound (allowed 2): " + ", ".join(f"{k} {v:.3g}" for k, v in ratios.items()))
    wide = {k: _worst(got[k] - ref[r], bound["expanded"][k]) for k, r in (("bp", "bp"), ("bl", "bl"), ("cost", "cost_pose"))}
    print("    for the record, against the bound with the residual expanded into m - u: " + ", ".join(f"{k} {v:.3g}" for k, v in wide.items()))
    assert max(ratios.values()) <= 2.0, ratios
    assert abs(cost - ref["cost"]) <= 2 * bound["cost"].sum()


# ---- cases 4 and 6: reduce and back-substitution on integer blocks ------------------------------------------------------------
def _upload_blocks(prob, blk):
    f = lambda a: np.ascontiguousarray(a, np.float64)
    prob.d_Hpl.upload(f(blk["Hpl"]).reshape(-1, 18))
    prob.d_Hll.upload(f(C.packed(blk["Hll"], C.TRI3)))
    prob.d_bl.upload(f(blk["bl"]))
    prob.d_Hpp.upload(f(C.packed(blk["Hpp"], C.TRI)))
    prob.d_bp.upload(f(blk["bp"]))
    prob.d_dp.upload(f(blk["dp"]))


def _backsub(prob):
    c = prob.ctx
    prob._check(c.lib.slam_bas_backsub_f64(c.handle, prob.K, prob.L, prob.O, prob.d_pt_ptr.ptr, prob.d_pt_obs.ptr, prob.d_op.ptr, prob.d_Hpl.ptr,
                                           prob.d_E.ptr, prob.d_bl.ptr, prob.d_dp.ptr, prob.d_dl.ptr))
    return prob.d_dl.download(np.float64, (prob.L, 3))


@pytest.mark.parametrize("lam", [0, 1])
@pytest.mark.parametrize("name", ["long-e7", "long-e8", "hub41"])
def test_reduce_and_backsub_on_integer_blocks_are_exact(gpu_ctx, name, lam):
    """The index tables of the layout with integer blocks uploaded in place of a linearisation: E, E bl, W, Hdiag (the full
    6x6: both triangles), b and dl equal the exact statement byte for byte, at lambda = 0 (Hll unimodular) and lambda = 1
    (Hll + I unimodular).  E, E bl and dl are 0 for the points nobody observes.  dl takes dp of the observing pose as given,
    fixed or not (dp is non-zero on the fixed pose here).  long: edges of 63, 64, 65, 128, 129 and 1 pairs, poses of up to
    1468 observations; hub41: a point seen by 41 poses (780 edges of one pair more), tracks of 1."""
    lay = {"long-e7": lambda: C.long_layout("e7"), "long-e8": lambda: C.long_layout("e8"), "hub41": C.hub_layout}[name]()
    from slamhip import SparseBAProblem

    K, L = lay["K"], len(lay["tracks"])
    op, ol = C.observations(lay["tracks"], 31)
    fixed = np.arange(K) == 0
    blk = C.integer_blocks(K, L, op, ol, lam, 31)
    cov = R.brute_covisibility(op, ol, K, fixed)
    ex = C.reduce_exact(blk, cov)
    prob = SparseBAProblem(gpu_ctx, K, L, op, ol, np.zeros((len(op), 2)), C.GRID_INTR, fixed)
    try:
        assert [tuple(e) for e in prob.edges.tolist()] == ex["keys"]
        _upload_blocks(prob, blk)
        prob.reduce(float(lam))
        Hd, W, b = prob.reduced_system()
        E, Ebl = prob.d_E.download(np.float64, (L, 9)), prob.d_Ebl.download(np.float64, (L, 3))
        dl = _backsub(prob)
    finally:
        prob.free()
    for what, got in (("E", E), ("Ebl", Ebl), ("W", W.reshape(-1, 36)), ("Hdiag", Hd.reshape(K, 36)), ("b", b), ("dl", dl)):
        assert C.same_bits(got, ex[what]), (what, int((got != ex[what]).sum()))
    assert np.array_equal(Hd, Hd.transpose(0, 2, 1)) and not np.array_equal(Hd, np.triu(Hd))
    unseen = ~blk["seen"]
    assert unseen.sum() >= 2 and not E[unseen].any() and not Ebl[unseen].any() and not dl[unseen].any()
    assert blk["dp"][0].all() and fixed[0]


# ---- the raw entry points on guarded buffers ------------------------------------------------------------------------------
MARGIN = 8                                                        # rows of bait on either side of every array
BAIT = np.frombuffer(struct.pack("<Q", 0x7FF8DEADBEEF0001), np.float64)[0]     # a NaN no kernel produces
_BAITS = {np.dtype(np.float64): BAIT, np.dtype(np.int32): 0, np.dtype(np.uint8): 1}   # an index read from bait stays in range


class Guarded:
    """Device arrays that each lie inside a larger allocation, MARGIN rows of bait before and after.  `get` checks the bait."""

    def __init__(self, ctx):
        self.ctx, self.arrays = ctx, {}

    def put(self, name, host):
        host = np.ascontiguousarray(host)
        rows = host.reshape(len(host), -1)
        full = np.full((len(rows) + 2 * MARGIN, rows.shape[1]), _BAITS[host.dtype], host.dtype)
        full[MARGIN:MARGIN + len(rows)] = rows
        self.arrays[name] = (self.ctx.upload(full), full, host.shape)
        return self

    def new(self, name, shape):
        return self.put(name, np.full(shape, BAIT, np.float64))

    def ptr(self, name):
        buf, full, _ = self.arrays[name]
        return buf.ptr + MARGIN * full.shape[1] * full.itemsize

    def get(self, name):
        buf, full, shape = self.arrays[name]
        now = buf.download(full.dtype, full.shape)
        assert now[:MARGIN].tobytes() == full[:MARGIN].tobytes() and now[-MARGIN:].tobytes() == full[-MARGIN:].tobytes(), f"bait of {name} touched"
        return now[MARGIN:-MARGIN].reshape(shape)

    def free(self):
        for buf, _, _ in self.arrays.values():
            buf.free()
        self.arrays = {}


def _tables(K, L, op, ol, fixed):
    from slamhip import covisibility
    from slamhip.ba import observation_lists

    edges, _, pair_ptr, pair_a, pair_b = covisibility(op, ol, K, fixed, L)
    pt_ptr, pt_obs, ps_ptr, ps_obs = observation_lists(op, ol, K, L)
    return dict(obs_pose=np.asarray(op, np.int32), obs_point=np.asarray(ol, np.int32), pt_ptr=pt_ptr, pt_obs=pt_obs, ps_ptr=ps_ptr, ps_obs=ps_obs,
                pair_ptr=pair_ptr, pair_a=pair_a, pair_b=pair_b, edges=edges)


OUTPUTS = ("Hpl", "Hll", "bl", "Hpp", "bp", "cost", "E", "Ebl", "Hdiag", "W", "b", "dl", "cost2")


def _raw_run(ctx, sc, tab, dp, delta, lam):
    """linearize, reduce, backsub and cost through the C ABI on guarded buffers -> (outputs, index errors counted, scalars)."""
    K, L, O, E, P = sc["K"], sc["L"], len(sc["op"]), len(tab["pair_ptr"]) - 1, len(tab["pair_a"])
    g = Guarded(ctx)
    try:
        for name in ("obs_pose", "obs_point", "pt_ptr", "pt_obs", "ps_ptr", "ps_obs", "pair_ptr", "pair_a", "pair_b"):
            g.put(name, tab[name])
        g.put("meas", sc["meas"]).put("T", sc["T12"]).put("X", sc["X"]).put("fixed", sc["fixed"].astype(np.uint8)).put("dp", np.asarray(dp, np.float64))
        for name, shape in (("Hpl", (O, 18)), ("Hll", (L, 6)), ("bl", (L, 3)), ("Hpp", (K, 21)), ("bp", (K, 6)), ("cost", (K,)), ("E", (L, 9)),
                            ("Ebl", (L, 3)), ("Hdiag", (K, 36)), ("W", (E, 36)), ("b", (K, 6)), ("dl", (L, 3)), ("cost2", (K,)), ("scal", (8,))):
            g.new(name, shape)
        p, lib, h = g.ptr, ctx.lib, ctx.handle
        _index_errors(ctx)
        intr = [float(v) for v in sc["intr"]]
        rc = [lib.slam_bas_linearize_f64(h, K, L, O, p("T"), p("X"), p("obs_pose"), p("obs_point"), p("meas"), p("pt_ptr"), p("pt_obs"), p("ps_ptr"),
                                         p("ps_obs"), p("fixed"), *intr, float(delta), p("Hpl"), p("Hll"), p("bl"), p("Hpp"), p("bp"), p("cost"), p("scal")),
              lib.slam_bas_reduce_f64(h, K, L, O, E, P, p("obs_point"), p("pt_ptr"), p("ps_ptr"), p("ps_obs"), p("pair_ptr"), p("pair_a"), p("pair_b"),
                                      p("Hpl"), p("Hll"), p("bl"), p("Hpp"), p("bp"), float(lam), p("E"), p("Ebl"), p("Hdiag"), p("W"), p("b")),
              lib.slam_bas_backsub_f64(h, K, L, O, p("pt_ptr"), p("pt_obs"), p("obs_pose"), p("Hpl"), p("E"), p("bl"), p("dp"), p("dl")),
              lib.slam_bas_cost_f64(h, K, L, O, p("T"), p("X"), p("obs_pose"), p("obs_point"), p("meas"), p("ps_ptr"), p("ps_obs"), *intr, float(delta),
                                    p("cost2"), p("scal") + 24)]
        assert rc == [0, 0, 0, 0], rc
        errors = _index_errors(ctx)
        out = {name: g.get(name) for name in OUTPUTS}
        scal = g.get("scal")
        for name in ("obs_pose", "obs_point", "pt_ptr", "pt_obs", "ps_ptr", "ps_obs", "pair_ptr", "pair_a", "pair_b", "meas", "T", "X", "fixed", "dp"):
            assert g.get(name).tobytes() == np.ascontiguousarray(g.arrays[name][1][MARGIN:-MARGIN]).tobytes(), name
        return out, errors, scal
    finally:
        g.free()


def _guard_base(ctx):
    def make():
        sc = C.grid_scene(C.long_layout(), 21)
        tab = _tables(sc["K"], sc["L"], sc["op"], sc["ol"], sc["fixed"])
        dp = np.random.default_rng(3).integers(-3, 4, (sc["K"], 6)).astype(np.float64)
        clean, errors, scal = _raw_run(ctx, sc, tab, dp, 5.0, 1.0)
        assert errors == 0
        return sc, tab, dp, clean, scal
    return _once("guard-base", make)


def test_raw_entries_on_guarded_buffers_equal_the_exact_statement(gpu_ctx):
    """The clean run of the guard tests: through the C ABI with every array inside bait, the linearisation equals the
    Fraction statement, the candidate's cost array equals the linearisation's, nothing is counted, no bait is touched."""
    sc, tab, dp, clean, scal = _guard_base(gpu_ctx)
    ex = C.linearize_exact(sc, 5.0)
    for name in ("Hpl", "Hll", "bl", "Hpp", "bp", "cost"):
        assert C.same_bits(clean[name], ex[name]), name
    assert C.same_bits(clean["cost2"], ex["cost"]) and _f64bits(scal[0]) == _f64bits(scal[3]) == _f64bits(int(ex["total"]))
    assert all(np.isfinite(clean[name]).all() for name in OUTPUTS)


def _corruptions(sc, tab):
    """name -> (table, index, value, what): one entry of one table replaced."""
    K, L, O = sc["K"], sc["L"], len(sc["op"])
    E, P = len(tab["pair_ptr"]) - 1, len(tab["pair_a"])
    o = int(np.flatnonzero(sc["op"] == 5)[40])
    out = {}
    for name, idx, n in (("obs_pose", o, K), ("obs_point", o, L), ("pt_obs", int(tab["pt_ptr"][sc["ol"][o]]), O), ("ps_obs", int(tab["ps_ptr"][3]) + 7, O),
                         ("pair_a", int(tab["pair_ptr"][2]) + 5, O), ("pair_b", int(tab["pair_ptr"][4]) + 70, O)):
        out[f"{name}=-1"] = (name, idx, -1)
        out[f"{name}=len"] = (name, idx, n)
    for name, j, n in (("pt_ptr", 100, O), ("ps_ptr", 3, O), ("pair_ptr", 2, P)):
        last = len(tab[name]) - 1
        out[f"{name} negative"] = (name, j, -3)
        out[f"{name} descending"] = (name, j, int(tab[name][j + 1]) + 2)
        out[f"{name} past the end"] = (name, last, n + 1)
    return out


CORRUPTIONS = [f"{t}={v}" for t in ("obs_pose", "obs_point", "pt_obs", "ps_obs", "pair_a", "pair_b") for v in ("-1", "len")] + \
              [f"{t} {v}" for t in ("pt_ptr", "ps_ptr", "pair_ptr") for v in ("negative", "descending", "past the end")]


@pytest.mark.parametrize("which", CORRUPTIONS)
def test_one_corrupt_index_is_contained(gpu_ctx, which):
    """One corruption in a copy of the long layout's tables, through the raw entries (the Python layer would refuse it).
    What the kernels' guards promise (the guard table):
      an entry of obs_pose / obs_point outside its range   counted once; Hpl_o, Hll[0] of its point, the cost of its pose NaN
      an entry of pt_obs outside [0, O)                    not counted; Hll[0] and dl of the point NaN
      an entry of ps_obs outside [0, O)                    not counted; cost, Hdiag[0] and the candidate cost of the pose NaN
      an entry of pair_a / pair_b outside [0, O)           counted once; W[0] of the edge NaN
      a slice of pt_ptr / ps_ptr outside the table         counted once per slice; the list is empty: the sums are 0
      a slice of pair_ptr outside the table                counted once per slice; W[0] of the edge NaN
    and everything the corruption does not feed is the clean run's, byte for byte; no bait is touched (checked by
    Guarded.get); the context runs the clean problem to the same bytes afterwards.  A pointer entry belongs to two slices,
    so `negative` counts twice; `descending` leaves its left neighbour a longer but valid slice (wrong numbers, not
    counted)."""
    sc, tab, dp, clean, _ = _guard_base(gpu_ctx)
    K, L, O = sc["K"], sc["L"], len(sc["op"])
    op, ol = sc["op"], sc["ol"]
    table, idx, value = _corruptions(sc, tab)[which]
    bad = {k: v.copy() for k, v in tab.items()}
    assert bad[table][idx] != value
    bad[table][idx] = value
    got, errors, _ = _raw_run(gpu_ctx, sc, bad, dp, 5.0, 1.0)

    isnan = np.isnan
    terms = _once("guard-terms", lambda: C.linearise_f64(sc, 5.0))

    def lacks(k, o):
        """Hpp and bp of pose k are the clean ones without the term of observation o - exactly, on this scene."""
        assert C.same_bits(got["Hpp"][k], clean["Hpp"][k] - C.packed(terms["Hpp"][o][None], C.TRI)[0])
        assert C.same_bits(got["bp"][k], clean["bp"][k] - terms["bp"][o])

    obs_t, pts, poses, edges_t, expect = set(), set(), set(), set(), 0
    pair_edge = np.searchsorted(tab["pair_ptr"], np.arange(len(tab["pair_a"])), side="right") - 1
    if table in ("obs_pose", "obs_point"):
        obs_t, pts, poses, expect = {idx}, {int(ol[idx])}, {int(op[idx])}, 1
        assert isnan(got["Hpl"][idx]).all() and isnan(got["Hll"][ol[idx], 0]) and isnan(got["cost"][op[idx]]) and isnan(got["cost2"][op[idx]])
        lacks(int(op[idx]), idx)
    elif table == "pt_obs":
        l = int(np.searchsorted(tab["pt_ptr"], idx, side="right") - 1)
        pts = {l}
        assert isnan(got["Hll"][l, 0]) and isnan(got["dl"][l]).any()
    elif table == "ps_obs":
        k = int(np.searchsorted(tab["ps_ptr"], idx, side="right") - 1)
        poses = {k}
        assert k == 3 and isnan(got["cost"][k]) and isnan(got["Hdiag"][k, 0]) and isnan(got["cost2"][k])
        lacks(k, int(tab["ps_obs"][idx]))
    elif table in ("pair_a", "pair_b"):
        edges_t, expect = {int(pair_edge[idx])}, 1
        assert isnan(got["W"][pair_edge[idx], 0])
    else:
        n = {"pt_ptr": O, "ps_ptr": O, "pair_ptr": len(tab["pair_a"])}[table]
        a0, a1 = bad[table][:-1].astype(np.int64), bad[table][1:].astype(np.int64)
        changed = np.flatnonzero((a0 != tab[table][:-1]) | (a1 != tab[table][1:]))
        corrupt = np.flatnonzero((a0 < 0) | (a1 < a0) | (a1 > n))
        assert set(corrupt) <= set(changed) and len(corrupt) == {"negative": 2, "descending": 1, "past the end": 1}[which.split(" ", 1)[1]]
        expect = len(corrupt)
        if table == "pt_ptr":
            pts = set(changed.tolist())
            for l in corrupt:
                assert not got["Hll"][l].any() and not got["bl"][l].any() and not got["dl"][l].any()
        elif table == "ps_ptr":
            poses = set(changed.tolist())
            for k in corrupt:
                assert not got["Hpp"][k].any() and not got["bp"][k].any() and got["cost"][k] == 0 and got["cost2"][k] == 0
                assert not got["Hdiag"][k].any() and not got["b"][k].any()
        else:
            edges_t = set(changed.tolist())
            for e in corrupt:
                assert isnan(got["W"][e, 0])
    assert errors == expect, (errors, expect)
    # what the corruption feeds: a point's E feeds every pose that sees it and every edge with a pair at it
    at = np.isin(ol, sorted(pts))
    poses |= set(op[at].tolist())
    edges_t |= set(pair_edge[np.isin(ol[tab["pair_a"]], sorted(pts)) | np.isin(tab["pair_a"], sorted(obs_t)) | np.isin(tab["pair_b"], sorted(obs_t))].tolist())
    keep = lambda n, touched: np.setdiff1d(np.arange(n), sorted(touched))
    rows = dict(Hpl=keep(O, obs_t), Hll=keep(L, pts), bl=keep(L, pts), E=keep(L, pts), Ebl=keep(L, pts), dl=keep(L, pts), Hpp=keep(K, poses), bp=keep(K, poses),
                cost=keep(K, poses), cost2=keep(K, poses), Hdiag=keep(K, poses), b=keep(K, poses), W=keep(len(tab["pair_ptr"]) - 1, edges_t))
    assert len(rows["Hpp"]) >= 2 and len(rows["W"]) >= 3 and len(rows["Hll"]) >= L - 3
    for name, r in rows.items():
        assert C.same_bits(got[name][r], clean[name][r]), name
    again, errors, _ = _raw_run(gpu_ctx, sc, tab, dp, 5.0, 1.0)
    assert errors == 0 and all(C.same_bits(again[name], clean[name]) for name in OUTPUTS)


def test_the_same_pair_list_at_five_edge_indices(gpu_ctx):
    """slam_bas_reduce_f64 with a pair table of the test's own: the 129-pair list of edge (1, 6) repeated as edges 0..4 - the
    four waves of a workgroup and the first wave of a second one.  Every W equals the exact block byte for byte."""
    lay = C.long_layout()
    K, L = lay["K"], len(lay["tracks"])
    op, ol = C.observations(lay["tracks"], 31)
    fixed = np.arange(K) == 0
    blk = C.integer_blocks(K, L, op, ol, 1, 31)
    cov = R.brute_covisibility(op, ol, K, fixed)
    ex = C.reduce_exact(blk, cov)
    want = ex["W"][ex["keys"].index((1, 6))]
    _, a, b = (np.array(v, np.int32) for v in zip(*cov[(1, 6)]))
    assert len(a) == 129
    tab = _tables(K, L, op, ol, fixed)
    g = Guarded(gpu_ctx)
    try:
        f = lambda x: np.ascontiguousarray(x, np.float64)
        g.put("pair_ptr", (129 * np.arange(6)).astype(np.int32)).put("pair_a", np.tile(a, 5)).put("pair_b", np.tile(b, 5))
        for name in ("obs_point", "pt_ptr", "ps_ptr", "ps_obs"):
            g.put(name, tab[name])
        g.put("Hpl", f(blk["Hpl"]).reshape(-1, 18)).put("Hll", f(C.packed(blk["Hll"], C.TRI3))).put("bl", f(blk["bl"]))
        g.put("Hpp", f(C.packed(blk["Hpp"], C.TRI))).put("bp", f(blk["bp"]))
        g.new("E", (L, 9)).new("Ebl", (L, 3)).new("Hdiag", (K, 36)).new("W", (5, 36)).new("b", (K, 6))
        p = g.ptr
        assert gpu_ctx.lib.slam_bas_reduce_f64(gpu_ctx.handle, K, L, len(op), 5, 5 * 129, p("obs_point"), p("pt_ptr"), p("ps_ptr"), p("ps_obs"), p("pair_ptr"),
                                               p("pair_a"), p("pair_b"), p("Hpl"), p("Hll"), p("bl"), p("Hpp"), p("bp"), 1.0, p("E"), p("Ebl"), p("Hdiag"),
                                               p("W"), p("b")) == 0
        W, Hd = g.get("W"), g.get("Hdiag")
    finally:
        g.free()
    for e in range(5):
        assert C.same_bits(W[e], want), e
    assert C.same_bits(Hd, ex["Hdiag"])


# ---- case 5: one free pose, E = 0 --------------------------------------------------------------------------------------------
def test_one_free_pose_without_an_edge(gpu_ctx):
    """ba_sparse_ref.smallest: K = 3, two fixed poses, E = 0 - slam_bas_reduce_f64 skips the edge kernel.  Hdiag and b against
    numpy within twice ba_sparse_ref.reduce's bound; six iterations against oracle.ba_lm_c with _holds' bars."""
    from slamhip import bundle_adjust_sparse

    w = R.smallest(np.random.default_rng(77))
    fixed, lam = np.array([True, True, False]), 2.5
    lin = R.linearize(_rt(w["T0"]), w["X0"], w["op"], w["ol"], w["meas"], R.INTR, 1.0)
    red = R.reduce(lin, w["op"], w["ol"], fixed, lam)
    prob = _window_problem(gpu_ctx, w)
    try:
        assert prob.E == 0 and prob.P == 0 and len(red["edges"]) == 0
        prob.linearize(1.0)
        prob.reduce(lam)
        Hd, b = prob.d_Hdiag.download(np.float64, (3, 6, 6)), prob.d_b.download(np.float64, (3, 6))
    finally:
        prob.free()
    ratios = dict(Hdiag=_worst(Hd[2] - red["Hdiag"][2], red["bound"]["Hdiag"][2]), b=_worst(b[2] - red["b"][2], red["bound"]["b"][2]))
    print(f"\none free pose, E = 0: |difference| / bound (allowed 2): {ratios}")
    assert max(ratios.values()) <= 2.0
    got, st = bundle_adjust_sparse(w["T0"], w["X0"], w["op"], w["ol"], w["meas"], R.INTR, iterations=6, fixed_poses=w["fixed"], huber_delta=1.0,
                                   pcg_tol=1e-10, ctx=gpu_ctx)
    ref = oracle.ba_lm_c(_rt(w["T0"]), w["X0"], w["op"], w["ol"], w["meas"], *R.INTR, 6, w["fixed"], 1.0)
    print(f"one free pose: poses {np.abs(got.poses - ref[0]).max():.3g}, points {np.abs(got.points - ref[1]).max():.3g}, stats {st}")
    _holds(got, ref, w)
    assert st["edges"] == 0 and st["unconverged"] == 0


# ---- case 7: the candidate ----------------------------------------------------------------------------------------------------
def _candidate(ctx, c):
    """slam_bas_candidate_f64 on guarded buffers of the test's own -> (T', X', denominator, partial sums)."""
    K, L = c["K"], c["L"]
    g = Guarded(ctx)
    try:
        g.put("fixed", c["fixed"].astype(np.uint8))
        for name in ("T", "X", "dp", "dl", "bp", "bl"):
            g.put(name, c[name])
        g.new("Tn", (K, 12)).new("Xn", (L, 3)).new("part", (1024,)).new("den", (1,))
        p = g.ptr
        assert ctx.lib.slam_bas_candidate_f64(ctx.handle, K, L, p("fixed"), p("T"), p("X"), p("dp"), p("dl"), p("bp"), p("bl"), c["lam"], p("Tn"), p("Xn"),
                                              p("part"), p("den")) == 0
        out = g.get("Tn"), g.get("Xn"), g.get("den")[0], g.get("part")
        for name in ("T", "X", "dp", "dl", "bp", "bl"):
            assert g.get(name).tobytes() == c[name].tobytes(), name
        return out
    finally:
        g.free()


@pytest.mark.parametrize("K,L", C.CANDIDATE_SHAPES)
def test_candidate_on_integer_steps_is_exact(gpu_ctx, K, L):
    """slam_bas_candidate_f64 at lambda = 2 on integers.  K + L = 262144 + 593 enters the grid-stride loop under the cap of
    1024 workgroups, and the finish kernel sums 1024 partials; 262144 is the last size without a second trip; 255, 256 and
    257 straddle one workgroup.  Byte for byte: X' = X + dl; T' = T + [0 | v] for the free poses (w = 0); the fixed poses
    come back as they went in although their dp and bp are not zero; the denominator equals the Python integer sum over
    the free poses and the points - the fixed poses' terms, not zero, are not in it; one partial per workgroup is written."""
    c = C.candidate_case(K, L, rotating=False)
    Tn, Xn, den, plain = C.candidate_exact(c)
    gT, gX, gden, part = _candidate(gpu_ctx, c)
    assert plain.all() and C.same_bits(gX, Xn) and C.same_bits(gT, Tn)
    assert C.same_bits(gT[c["fixed"]], c["T"][c["fixed"]]) and c["dp"][c["fixed"]].all() and c["bp"][c["fixed"]].all()
    blocks = min(1024, (K + L + 255) // 256)
    assert not np.isnan(part[:blocks]).any() and (blocks == 1024 or np.isnan(part[blocks:]).all())
    assert _f64bits(gden) == _f64bits(den), (gden, den)
    assert _f64bits(part[:blocks].sum()) == _f64bits(den)


@pytest.mark.parametrize("K,L", [C.CANDIDATE_SHAPES[0], C.CANDIDATE_SHAPES[3]])
def test_candidate_with_rotating_poses(gpu_ctx, K, L):
    """A few free poses turn by 0.5 to 1.5 rad: T' against oracle.se3_exp_np(dp) @ T within twice cases.update_bound, which
    counts roundings per entry from dp and T alone; everything else stays exact; the denominator is the integer part plus
    those poses' f64 terms within the roundings of adding them."""
    c = C.candidate_case(K, L)
    Tn, Xn, den, plain = C.candidate_exact(c)
    gT, gX, gden, _ = _candidate(gpu_ctx, c)
    assert C.same_bits(gX, Xn) and C.same_bits(gT[plain], Tn[plain]) and not plain.all()
    worst = 0.0
    for k in c["rot"]:
        want = (oracle.se3_exp_np(c["dp"][k]) @ np.vstack([c["T"][k].reshape(3, 4), [0, 0, 0, 1]]))[:3].reshape(12)
        worst = max(worst, _worst(gT[k] - want, C.update_bound(c["dp"][k], c["T"][k])))
    extra = np.array([d * (c["lam"] * d - b) for k in c["rot"] for d, b in zip(c["dp"][k], c["bp"][k])])
    slack = (len(extra) + 12) * R.EPS * (abs(den) + np.abs(extra).sum())
    print(f"\ncandidate K={K} L={L}: rotating poses |difference| / bound (allowed 2): {worst:.3g}; denominator off by "
          f"{abs(gden - (den + extra.sum())):.3g} of {slack:.3g} allowed")
    assert worst <= 2.0 and abs(gden - (den + extra.sum())) <= slack


# ---- case 8: the cost identity ---------------------------------------------------------------------------------------------------
def test_accepted_candidate_cost_is_the_next_linearisation_cost(gpu_ctx):
    """slam_bas_cost_f64 sums as bas_pose_kernel does, so an accepted candidate's cost equals the next
    linearisation's bit for bit - the total and the per-pose array, on the long layout (poses of up to 1468 observations)."""
    w = _once("long-window", lambda: C.random_window(C.long_layout()))
    prob = _window_problem(gpu_ctx, w)
    try:
        cost, dmax = prob.linearize(1.0)
        lam, accepted = 1e-5 * dmax, False
        for _ in range(10):
            prob.reduce(lam)
            if prob.solve(lam, 1e-10, 500)["converged"]:
                den, new = prob.step(lam, 1.0)
                if np.isfinite(new) and (cost - new) / (den + 1e-3) > 0:
                    accepted = True
                    break
            lam *= 4
        assert accepted, "no accepted trial in ten"
        cand = prob.d_cost2.download(np.float64, (prob.K,))
        prob.accept()
        again, _ = prob.linearize(1.0)
        per_pose = prob.d_cost.download(np.float64, (prob.K,))
    finally:
        prob.free()
    print(f"\ncost identity: {cost:.17g} -> {new:.17g} at lambda {lam:.3g}")
    assert new < cost and _f64bits(again) == _f64bits(new) and per_pose.tobytes() == cand.tobytes()


# ---- case 9: placement -------------------------------------------------------------------------------------------------------------
def test_blocks_do_not_depend_on_where_the_problem_lies(gpu_ctx):
    """The long layout alone, and embedded among 40 extra poses and 500 extra points (relabelled so that every list keeps its
    order): Hpp, bp, cost, Hdiag, b of every original pose, Hll, bl of every original point and W of every original edge
    are the same bytes - other workgroups, other waves of the edge kernel, other threads of the point kernels."""
    w = _once("long-window", lambda: C.random_window(C.long_layout()))
    big, pm, lm, om = C.embed(w)
    res = []
    for win in (w, big):
        prob = _window_problem(gpu_ctx, win)
        try:
            prob.linearize(1.0)
            prob.reduce(2.5)
            Hd, W, b = prob.reduced_system()
            res.append(dict(_lin_blocks(prob), Hdiag=Hd, W=W, b=b, edges=prob.edges.copy()))
        finally:
            prob.free()
    a, b = res
    where = {tuple(e): i for i, e in enumerate(b["edges"].tolist())}
    em = np.array([where[(int(pm[k1]), int(pm[k2]))] for k1, k2 in a["edges"].tolist()])
    assert len(em) == 7 and not np.array_equal(em, np.arange(7))
    for name, m in (("Hpp", pm), ("bp", pm), ("cost", pm), ("Hdiag", pm), ("b", pm), ("Hll", lm), ("bl", lm), ("Hpl", om), ("W", em)):
        assert a[name].tobytes() == np.ascontiguousarray(b[name][m]).tobytes(), name
