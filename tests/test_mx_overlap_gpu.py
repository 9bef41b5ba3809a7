"""GPU: the overlapped scan loop of the matrix-core top-2 search (bf_mx.hip: a group's A operands are read behind the MFMAs
of the group before it, and a whole stage that another follows expands and stores that next stage between the MFMAs of its
groups 4-7, one source word per group), engine 2 against the VALU kernel (engine 1) and oracle.bf_knn_c, bit for bit.

Every case asserts its plan against tests/test_mx_overlap_cpu.expected_plan (the planner's documented rule), because which
path a stage takes follows from the plan alone:
  * a chunk of one stage never stages in the shadow (it stores at the chunk start only) and reads ahead inside trips of four
    groups; a short stage runs what the trips leave with the test for rows past the chunk;
  * in a chunk of several stages every stage but the last is whole, runs as one trip of eight and carries the next stage's
    store.  (The planner's tails shrink to chunks of one stage, so a short stage is always a chunk of its own and is staged at
    its chunk start; the kernel's clamp for a short stage staged in the shadow is a guard no plan reaches.)
As tests/test_mx_ties_gpu.py this module shows agreement; the rules themselves are pinned by the CPU suites."""
import numpy as np
import pytest

from oracle import oracle
from hamming_families import expected_topk, prefix_rows
from test_mx_overlap_cpu import expected_plan
from test_mx_ties_gpu import few_values, plan, same, search

pytestmark = pytest.mark.gpu

STAGE = 128


def check_plan(ctx, n, m):
    p, tbl = plan(ctx, n, m)
    want, wtbl = expected_plan(ctx.plan_info(n, m)["cus"], n, m)
    assert p == want and tbl == wtbl
    return p, tbl


def run(ctx, q, t, ref=None, twice=False):
    """Engine 2 against engine 1 and the reference (the oracle unless given); returns engine 2's table."""
    import slamhip

    n, m = len(q), len(t)
    if ref is None:
        ref = oracle.bf_knn_c(q, t, 2, threads=16)
    dq, dt = slamhip.DeviceDescriptors(ctx, q), slamhip.DeviceDescriptors(ctx, t)
    try:
        mx = search(ctx, dq, n, dt, m, 2)
        if twice:                                   # nothing of a launch may survive into the next one on the same context
            assert same(search(ctx, dq, n, dt, m, 2), mx)
        valu = search(ctx, dq, n, dt, m, 1)
    finally:
        dq.free()
        dt.free()
    assert same(mx, ref)
    assert same(mx, valu)
    return mx


def random_rows(seed, n, m):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (n, 32), dtype=np.uint8), rng.integers(0, 256, (m, 32), dtype=np.uint8)


@pytest.mark.parametrize("m", [127, 128, 129, 255, 256, 257, 383, 384, 385, 1151])
@pytest.mark.parametrize("n", [64, 300])
def test_stage_edges(gpu_ctx, n, m):
    """Chunks of one stage: a whole stage alone, a whole stage and a short one of 1 or 127 rows in the next chunk, a short
    stage with fewer than one whole trip (M = 385: one row; M = 127, 255, 383, 1151: seven whole groups and one of 15)."""
    p, tbl = check_plan(gpu_ctx, n, m)
    assert tbl == list(range(0, m, STAGE)) + [m] and p["qblocks"] == (n + 255) // 256
    q, t = random_rows(1000 * n + m, n, m)
    run(gpu_ctx, q, t, twice=True)


@pytest.mark.parametrize("n,m,workers,chunk", [(16384, 16384, 16, 256), (16384, 16384 + 77, 16, 256), (65536, 32768, 4, 1024)])
def test_multi_stage_chunks_on_random_rows(gpu_ctx, n, m, workers, chunk):
    """Staging in the shadow: chunks of two and of eight stages, a tail that shrinks to single stages, and (M = 16384 + 77) a
    short last chunk.  Random rows: a word expanded into the wrong place moves nearly every distance."""
    p, tbl = check_plan(gpu_ctx, n, m)
    if gpu_ctx.plan_info(n, m)["cus"] == 256:
        assert (p["workers"], p["chunk"]) == (workers, chunk)
    assert max(b - a for a, b in zip(tbl, tbl[1:])) == p["chunk"] and p["chunk"] >= 2 * STAGE
    assert tbl[-1] - tbl[-2] == (m % STAGE or STAGE)
    q, t = random_rows(n + m, n, m)
    run(gpu_ctx, q, t, twice=True)


def test_planted_neighbours_at_the_rows_the_overlap_touches(gpu_ctx):
    """65536 x 32768, chunks of eight stages.  Position k (a stage-local row among the first and last rows of the groups whose
    shadow carries a store and of the groups at a trip's ends; the first, a middle and the last stage of a chunk; the first chunk
    of the table and the last one of at least three stages) holds the prefix row 2 k; every other train row is at least 54 bits from every query.  A
    query 2 k has its nearest row at position k and a TIE at distance 2 between the positions before and after it; a query
    2 k + 1 ties at distance 1 between positions k and k + 1 and at distance 3 behind them.  The lower row wins each tie."""
    n, m = 65536, 32768
    p, tbl = check_plan(gpu_ctx, n, m)
    assert p["chunk"] == 1024 and tbl[1] == 1024
    last = max(i for i in range(len(tbl) - 1) if tbl[i + 1] - tbl[i] >= 3 * STAGE)
    assert last > 8
    local = (0, 15, 16, 63, 64, 111, 112, 127)
    rng = np.random.default_rng(32768)
    a = rng.integers(150, 257, m)
    pos = []
    for c0, c1 in ((tbl[0], tbl[1]), (tbl[last], tbl[last + 1])):
        nst = (c1 - c0) // STAGE
        for st in (0, nst // 2, nst - 1):
            pos += [c0 + st * STAGE + r for r in local]
    assert len(set(pos)) == 48
    a[pos] = 2 * np.arange(48)
    b = rng.integers(0, 96, n)
    want = expected_topk(a, b, 2)
    # the data does what the docstring says
    j = int(np.nonzero(b == 2 * 20)[0][0])
    assert want[0][j].tolist() == [pos[20], pos[19]] and want[1][j].tolist() == [0, 2]
    j = int(np.nonzero(b == 2 * 20 + 1)[0][0])
    assert want[0][j].tolist() == [pos[20], pos[21]] and want[1][j].tolist() == [1, 1]
    mx = run(gpu_ctx, prefix_rows(b), prefix_rows(a), ref=want, twice=True)
    assert np.isin(mx[0], pos).all()


def test_exchanges_between_workers_on_few_valued_rows(gpu_ctx):
    """16 workers, 2048 rows each in chunks of two stages, the early exchange after a worker's first stage active; every
    distance is one of five values, so a stale or skipped exchange would let a losing tie through or drop a winning one."""
    n, m = 16384, 32768
    p, tbl = check_plan(gpu_ctx, n, m)
    assert p["workers"] > 1 and m // p["workers"] >= 1024 and p["chunk"] >= 2 * STAGE
    q, t = few_values(np.random.default_rng(5), n, m)
    run(gpu_ctx, q, t, twice=True)
