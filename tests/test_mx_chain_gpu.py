"""GPU: the chunk starts and the ticket path of the matrix-core top-2 search (bf_mx.hip), engine 2 against the VALU kernel
(engine 1) and oracle.bf_knn_c (or the exact table of the prefix family), bit for bit, every search twice on one context.

Which path a chunk takes follows from the plan alone, so every case asserts its plan against the documented rule
(tests/test_mx_overlap_cpu.expected_plan) and then the property of the table it is about:
  * only one-stage chunks: N = 64 and 300 with M up to 8269 - with so few queries the planner gives 256 workers and the tail
    rule shrinks every chunk to one stage; there are as many workers as chunks, so every worker's second ticket lies past the
    table (ticket exhaustion: the last chunk's successor does not exist);
  * two-stage chunks followed by a one-stage tail: with N = 64 or 300 the planner keeps a 256-row chunk only while
    (rest / 512) >= 256, so the nearest M to the small sizes that has such a table is 131072 + 255 ... 131072 + 513;
  * eight-stage chunks with a tail (and chunks of 7 ... 2 stages in between): N = 64, M = 2^21 + 1024 + 77;
  * a ragged last stage is always a one-stage chunk of its own behind other one-stage chunks in the planner's tables, so no
    shape reaches "a ragged stage handed over by a chunk of several stages"; tests/test_mx_chain_cpu.py drives that table.
The planted-row and threshold cases use tests/hamming_families.prefix_rows, where the distance of a query b to a row a is
|a - b| and the exact table is known without a search.

This module shows agreement; the rules are pinned by tests/test_mx_chain_cpu.py and tests/test_mx_ties_cpu.py."""
import numpy as np
import pytest

from hamming_families import expected_topk, prefix_rows
from test_mx_overlap_gpu import check_plan, random_rows, run

pytestmark = pytest.mark.gpu

STAGE = 128


def lens_of(tbl):
    return [b - a for a, b in zip(tbl, tbl[1:])]


@pytest.mark.parametrize("m", [255, 256, 257, 383, 384, 385, 511, 513, 1151, 2048 + 1, 8192 + 77])
@pytest.mark.parametrize("n", [64, 300])
def test_one_stage_chunks_and_ticket_exhaustion(gpu_ctx, n, m):
    p, tbl = check_plan(gpu_ctx, n, m)
    assert tbl == list(range(0, m, STAGE)) + [m]
    assert p["workers"] == p["chunks"] == (m + STAGE - 1) // STAGE        # every second ticket is past the table
    q, t = random_rows(7000 * n + m, n, m)
    run(gpu_ctx, q, t, twice=True)


@pytest.mark.parametrize("m", [131072 + 255, 131072 + 256, 131072 + 257, 131072 + 513])
@pytest.mark.parametrize("n", [64, 300])
def test_two_stage_chunks_then_a_one_stage_tail(gpu_ctx, n, m):
    p, tbl = check_plan(gpu_ctx, n, m)
    lens = lens_of(tbl)
    two = [i for i, ln in enumerate(lens) if ln == 2 * STAGE]
    assert p["chunk"] == 2 * STAGE and two and two == list(range(len(two)))      # two-stage chunks at the head ...
    assert set(lens[len(two):-1]) == {STAGE} and lens[-1] == (m % STAGE or STAGE)  # ... then single stages, the last one ragged
    assert p["workers"] > 1
    q, t = random_rows(n + m, n, m)
    run(gpu_ctx, q, t, twice=True)


def test_eight_stage_chunks_with_a_shrinking_tail(gpu_ctx):
    n, m = 64, (1 << 21) + 1024 + 77
    p, tbl = check_plan(gpu_ctx, n, m)
    lens = lens_of(tbl)
    assert p["chunk"] == 8 * STAGE and lens[0] == 8 * STAGE
    assert {7 * STAGE, 2 * STAGE, STAGE} <= set(lens) and lens[-1] == 77
    q, t = random_rows(n + m, n, m)
    run(gpu_ctx, q, t, twice=True)


@pytest.mark.parametrize("n,m,workers", [((1 << 18) + 3, 4096, 1), (16384, 16384, 16)])
def test_planted_neighbours_around_chunk_starts(gpu_ctx, n, m, workers):
    """Two-stage chunks, one worker (the next chunk is the adjacent one) and 16 workers (it is not).  Position k - the first
    and last row of a chunk, of its first stage and of its last stage, and the last row of the first group and the first row of
    the second group after a chunk start, in the first, a middle and the last two-stage chunk - holds the prefix row 2 k; every
    other train row is at least 54 bits from every query.  A query 2 k has its nearest row at position k and a TIE at distance 2
    between the positions before and after it; a query 2 k + 1 ties at distance 1 between positions k and k + 1.  The lower
    row wins each tie."""
    p, tbl = check_plan(gpu_ctx, n, m)
    lens = lens_of(tbl)
    two = [i for i, ln in enumerate(lens) if ln == 2 * STAGE]
    assert p["chunk"] == 2 * STAGE and len(two) >= 3
    if gpu_ctx.plan_info(n, m)["cus"] == 256:
        assert p["workers"] == workers
    pos = []
    for i in (two[0], two[len(two) // 2], two[-1]):
        c0, c1 = tbl[i], tbl[i + 1]
        pos += [c0, c0 + 15, c0 + 16, c0 + STAGE - 1, c0 + STAGE, c1 - 1]
    assert len(set(pos)) == 18 and pos == sorted(pos)
    rng = np.random.default_rng(m + workers)
    a = rng.integers(150, 257, m)
    a[pos] = 2 * np.arange(18)
    b = rng.integers(0, 36, n)
    want = expected_topk(a, b, 2)
    j = int(np.nonzero(b == 2 * 7)[0][0])
    assert want[0][j].tolist() == [pos[7], pos[6]] and want[1][j].tolist() == [0, 2]
    j = int(np.nonzero(b == 2 * 7 + 1)[0][0])
    assert want[0][j].tolist() == [pos[7], pos[8]] and want[1][j].tolist() == [1, 1]
    mx = run(gpu_ctx, prefix_rows(b), prefix_rows(a), ref=want, twice=True)
    assert np.isin(mx[0], pos).all()


def moving_threshold_rows(m):
    """Train values for queries of value 0 in tile 0 (queries 0-15 of every 64) and 90 in tile 1: in the chunk's first two
    stages a row of one group lowers the lane's threshold, and the group behind it holds, in the same tile and lane, a row that
    passes the old threshold but not the new one, a row that passes both and a tie at the new 2nd-best distance, and in another
    tile a passing row - at the last group of a trip (stage 0 group 7 -> stage 1 group 0) and at groups 0 -> 1, 3 -> 4, 6 -> 7."""
    a = np.full(m, 256, np.int64)
    at = lambda stage, g, pos: stage * STAGE + 16 * g + pos
    a[at(0, 0, 0)], a[at(0, 0, 1)] = 60, 55            # the pair (55, 60)
    a[at(0, 7, 2)] = 45                                # lowers to (45, 55): e = 54
    for g, lower in ((3, 35), (6, 25)):
        a[at(1, g, 2)] = lower
    for g, (old_only, both, tie), other in ((0, (57, 42, 55), 89), (1, (50, 40, 45), 88), (4, (41, 30, 40), 87), (7, (33, 20, 30), 86)):
        a[at(1, g, 0)], a[at(1, g, 1)], a[at(1, g, 2)] = old_only, both, tie
        a[at(1, g, 8)] = other
    return a


@pytest.mark.parametrize("n,m", [(64, 131072 + 256), (16384, 16384), (64, 256)])
def test_threshold_moves_in_the_group_before(gpu_ctx, n, m):
    p, tbl = check_plan(gpu_ctx, n, m)
    assert tbl[1] == (2 * STAGE if m > 256 else STAGE)            # m = 256: trips of four, a trip ends at groups 3 and 7
    a = moving_threshold_rows(m)
    b = np.array([0, 90, 45, 60])[(np.arange(n) // 16) % 4]
    want = expected_topk(a, b, 2)
    assert want[0][0].tolist() == [STAGE + 16 * 7 + 1, STAGE + 16 * 6 + 2] and want[1][0].tolist() == [20, 25]
    assert want[1][16].tolist() == [1, 2]
    run(gpu_ctx, prefix_rows(b), prefix_rows(a), ref=want, twice=True)
