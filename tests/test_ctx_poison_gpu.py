"""The state contract of the context blocks on the device ("State contract of the context blocks"): a call's result
depends on its arguments alone - not on what an earlier call left in the context's grow-only blocks, and not on what an output
buffer or a caller-owned workspace held before the call.

For every case of tests/ctx_poison_cases.py: the clean result on a fresh context is what the family's reference gives (the
baseline - nothing below compares the code with itself only); then the workspace, the io arena (device and pinned) and the
radius tables are filled with 0x00, 0xFF and 0x7F by slam_ctx_block_fill, every buffer the wrapper allocates is filled with
the same byte before its inputs are uploaded over it, and every output must come out with the baseline's bits over its whole
documented extent.  The same on blocks that do not exist yet, right after the workspace has moved, and with all cases
interleaved on one context."""
import ctypes

import numpy as np
import pytest

import ctx_poison_cases as T

pytestmark = pytest.mark.gpu

SCRATCH = ("workspace", "io_dev", "io_host", "radius_tables")
_baseline = {}


def poisoned(ctx, byte, monkeypatch):
    """The scratch blocks of the context filled with ``byte``, and every buffer ``ctx.malloc`` hands out from now on filled
    with it first: the wrappers upload their inputs over the fill, so outputs and caller-owned workspaces keep it."""
    from slamhip._lib import check
    from slamhip.device import Context

    for name in SCRATCH:
        ctx.fill_block(name, byte)
    real = Context.malloc.__get__(ctx)

    def filled(nbytes):
        b = real(nbytes)
        check(ctx.lib.slam_memset(ctx.handle, b.ptr, byte, b.nbytes))
        return b

    monkeypatch.setattr(ctx, "malloc", filled, raising=False)


def grow(ctx, case, scale=1):
    """A larger call of another family than the case's, so that every block exists and is larger than the case needs (and,
    for the graph solvers, a larger graph first: the case then finds every region of its layout inside another's)."""
    import slamhip

    if case.before is not None:
        case.before(ctx)

    rng = np.random.default_rng(77)
    n, m = 1500 * scale, 9000 * scale
    q, t = T._rows(rng, n), T._rows(rng, m)
    if case.file != "bf_window.hip":
        xy = rng.uniform(0, 640, (n + m, 2)).astype(np.float32)
        slamhip.window_match_arrays(q, t, xy[:n], xy[n:], 30.0, 2, ctx=ctx)          # workspace and io arena
    else:
        slamhip.topk_match_arrays(q, t, 7, ctx=ctx)
    if case.file != "bf_radius.hip":
        k = min(scale, 2)
        off, idx, dist = slamhip.radius_match_arrays(q[:1500 * k], t[:3000 * k], 105.0, ctx=ctx)   # radius tables (and the workspace: the emit's staging)
        assert off[-1] > 1500
    b = ctx.block_bytes()
    assert b["workspace"] > 0 and b["io_dev"] > 0 and b["io_host"] > 0 and (b["radius_tables"] > 0 or case.file == "bf_radius.hip"), b


def baseline(case):
    """The case's result on a fresh context of its own, checked against the family's reference."""
    import slamhip

    if case.name not in _baseline:
        ctx = slamhip.Context()
        try:
            outs = case.call(ctx)
            assert T.index_errors(ctx) == 0 and ctx.state_dirty() == 0
        finally:
            ctx.close()
        case.check(outs)
        _baseline[case.name] = case.masked(outs)
    return _baseline[case.name]


@pytest.fixture(scope="module")
def pctx(built):
    """The context every poisoned run of this file shares (the session's context stays as the suite's order left it)."""
    import slamhip

    ctx = slamhip.Context()
    yield ctx
    ctx.close()


@pytest.mark.parametrize("name", [c.name for c in T.CASES])
def test_clean_run_against_the_reference(built, name):
    baseline(T.BY_NAME[name])


@pytest.mark.parametrize("name", [c.name for c in T.CASES])
def test_poison_patterns(pctx, monkeypatch, name):
    case = T.BY_NAME[name]
    want = baseline(case)
    for byte in T.POISON_BYTES:
        grow(pctx, case)
        poisoned(pctx, byte, monkeypatch)
        got = case.masked(case.call(pctx))
        monkeypatch.undo()
        try:
            T.same(got, want)
        except AssertionError as e:
            raise AssertionError(f"{name}: the result changes when the blocks and the output buffers hold 0x{byte:02X}: {e}") from None
        assert T.index_errors(pctx) == 0, name
        if case.bf:
            assert pctx.state_dirty() == 0, name


@pytest.mark.parametrize("name", [c.name for c in T.CASES])
def test_pristine_blocks_and_a_moved_workspace(built, name):
    import slamhip

    case = T.BY_NAME[name]
    want = baseline(case)
    ctx = slamhip.Context()
    try:
        assert not any(ctx.block_bytes().values())
        T.same(case.masked(case.call(ctx)), want)
        before = ctx.block_bytes()["workspace"]
        for scale in (2, 8, 32):
            grow(ctx, case, scale=scale)
            if ctx.block_bytes()["workspace"] > before:
                break
        assert ctx.block_bytes()["workspace"] > before                # it grew, so it was freed and allocated again
        T.same(case.masked(case.call(ctx)), want)
    finally:
        ctx.close()


def test_all_cases_interleaved_twice_on_one_context(built):
    import slamhip

    order = [T.CASES[i] for i in np.random.default_rng(20261020).permutation(len(T.CASES))]
    want = {c.name: baseline(c) for c in order}
    ctx = slamhip.Context()
    try:
        for rnd in range(2):
            for case in order:
                try:
                    T.same(case.masked(case.call(ctx)), want[case.name])
                except AssertionError as e:
                    raise AssertionError(f"round {rnd}, {case.name} (order: {[c.name for c in order]}): {e}") from None
        assert ctx.state_dirty() == 0 and T.index_errors(ctx) == 0
    finally:
        ctx.close()


# ---- the hook itself ------------------------------------------------------------------------------------------------------
def test_hook_refuses_the_state_blocks_and_bad_indices(pctx):
    from slamhip._lib import SLAM_ERR_INVALID

    grow(pctx, T.BY_NAME["proj-project"])
    before = pctx.block_bytes()
    for block in (1, 2, 6, -1, 1 << 20):
        assert pctx.lib.slam_ctx_block_fill(pctx.handle, block, 0xFF) == SLAM_ERR_INVALID
        assert b"slam_ctx_block_fill" in pctx.lib.slam_last_error()
    assert pctx.lib.slam_ctx_block_fill(None, 0, 0xFF) == SLAM_ERR_INVALID
    with pytest.raises(ValueError):
        pctx.fill_block("no such block", 0)
    for name in ("merge_state", "pinned_block"):
        with pytest.raises(Exception, match="slam_ctx_block_fill"):
            pctx.fill_block(name, 0xFF)
    assert pctx.block_bytes() == before and pctx.state_dirty() == 0   # nothing changed: the merge state is still idle


def test_hook_on_untaken_blocks_is_a_no_op(built):
    import slamhip

    ctx = slamhip.Context()
    try:
        for name in SCRATCH:
            ctx.fill_block(name, 0x7F)
        assert not any(ctx.block_bytes().values())
        case = T.BY_NAME["proj-project"]
        T.same(case.masked(case.call(ctx)), baseline(case))
    finally:
        ctx.close()


def test_a_filled_workspace_and_the_projection_with_all_tables(pctx):
    case = T.BY_NAME["proj-project"]
    want = baseline(case)
    for byte in (0xFF, 0x00):
        case.call(pctx)                                                # the workspace exists and holds this call's pair table
        pctx.fill_block("workspace", byte)
        got = case.masked(case.call(pctx))
        T.same(got, want)
        case.check(got)


# ---- after the whole file --------------------------------------------------------------------------------------------------
def test_merge_state_and_index_errors_after_the_file(pctx):
    assert pctx.state_dirty() == 0
    assert T.index_errors(pctx) == 0
    n = ctypes.c_int64(-1)
    assert pctx.lib.slam_bf_state_dirty(pctx.handle, ctypes.byref(n)) == 0 and n.value == 0
