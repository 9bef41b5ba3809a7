"""GPU: the early bound exchanges of the matrix-core top-2 search (bf_mx.hip, SLAM_MX_EARLY: the workers of a query block
exchange after 128, 256 and 512 scanned rows, not only at chunk starts), engine 2 against the VALU kernel (engine 1), bit
for bit, on tie-heavy train sets: rows from a few byte values, and copies of one row placed on both sides of the 128-, 256-
and 512-row marks of the first chunks of different workers and of their chunk boundaries, so that a tie against another
worker's key has to be decided both ways.  Each case asserts its plan and runs once.

As tests/test_mx_ties_gpu.py this module shows AGREEMENT: which worker reads which bound depends on timing.  What pins the
rule is tests/test_mx_head_cpu.py, where the schedule is chosen."""
import numpy as np
import pytest

from test_mx_ties_gpu import few_values, plan, same, search

pytestmark = pytest.mark.gpu

MARKS = (0, 128, 256, 512)


def marked_copies(rng, n, m, tbl):
    """Random rows; several hundred queries get three copies of a row one bit away, each within 8 rows of a mark (the start,
    128, 256 or 512 rows into one of the first chunks of the table) or of the end of such a chunk, and a fourth anywhere."""
    q = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    t = rng.integers(0, 256, (m, 32), dtype=np.uint8)
    at = sorted({c0 + k for c0, c1 in zip(tbl[:12], tbl[1:13]) for k in MARKS if c0 + k < c1} | set(tbl[1:13]))
    pool = np.unique(np.clip(np.add.outer(np.array(at), np.arange(-8, 8)).ravel(), 0, m - 1))
    rng.shuffle(pool)
    cnt = min(n, len(pool) // 3)
    who = rng.choice(n, cnt, replace=False)
    v = q[who].copy()
    v[np.arange(cnt), rng.integers(0, 32, cnt)] ^= np.uint8(1) << rng.integers(0, 8, cnt).astype(np.uint8)
    t[rng.integers(0, m, cnt)] = v
    for j in range(3):
        t[pool[j * cnt:(j + 1) * cnt]] = v
    return q, t, cnt


# (n, m, chunk rows, workers per query block, chunks in the table)
REGIMES = [
    (65536, 32768, 1024, 4, None),          # the three early points inside a first chunk, and a later chunk start
    (8192, 65536, 256, 32, None),           # only the 128-row point falls inside a chunk
    (300, 1 << 21, 1024, 256, None),        # 256 workers: the first chunks cover 2^18 rows
    (65536, 384, 256, 3, 3),                # the train set ends inside the first chunks (single stages: no early point)
    (65536, 129, 256, 2, 2),
    (65536, 2048 + 300 + 5, 256, 4, None),  # a short queue: the 128-row point, then shrinking chunks and a ragged last stage
]


@pytest.mark.parametrize("fam", ["few_values", "marked_copies"])
@pytest.mark.parametrize("n,m,chunk,workers,chunks", REGIMES)
def test_early_exchanges_agree_with_the_valu_kernel(gpu_ctx, fam, n, m, chunk, workers, chunks):
    import slamhip

    ctx = gpu_ctx
    p, tbl = plan(ctx, n, m)
    assert p["chunk"] == chunk and p["workers"] == workers and p["stage_rows"] == 128 and tbl[0] == 0 and tbl[-1] == m
    assert chunks is None or p["chunks"] == chunks
    if chunks is None and m >= 32768:
        assert tbl[1] == chunk and tbl[workers] == workers * chunk      # every worker's first chunk is a uniform one
    rng = np.random.default_rng(n + m + len(fam))
    if fam == "few_values":
        q, t = few_values(rng, n, m)
        code = lambda a: a[:, :4].astype(np.int64) @ (1 << np.arange(0, 32, 8))
        rows, counts = np.unique(code(t), return_counts=True)
        want = int(np.isin(code(q), rows[counts >= 2]).sum())           # a query with two exact copies ties at distance 0
        assert want >= n // 2
    else:
        q, t, want = marked_copies(rng, n, m, tbl)
        want = want // 2                                                 # copies of different queries may share a row
    dq, dt = slamhip.DeviceDescriptors(ctx, q), slamhip.DeviceDescriptors(ctx, t)
    try:
        mx = search(ctx, dq, n, dt, m, 2)
        valu = search(ctx, dq, n, dt, m, 1)
    finally:
        dq.free()
        dt.free()
    assert same(mx, valu)
    idx, dist = mx
    tie = dist[:, 0] == dist[:, 1]
    assert tie.sum() >= want and (idx[tie, 0] < idx[tie, 1]).all()


def test_all_rows_equal(gpu_ctx):
    """Every pair ties: rows 0 and 1 win for every query, whatever any worker publishes from its 128th, 256th or 512th row."""
    import slamhip

    ctx = gpu_ctx
    n, m = 65536, 32768
    v = np.random.default_rng(5).integers(0, 256, 32, dtype=np.uint8)
    dq, dt = slamhip.DeviceDescriptors(ctx, np.tile(v, (n, 1))), slamhip.DeviceDescriptors(ctx, np.tile(v, (m, 1)))
    try:
        idx, dist = search(ctx, dq, n, dt, m, 2)
    finally:
        dq.free()
        dt.free()
    assert (idx == np.array([0, 1])).all() and (dist == 0).all()
