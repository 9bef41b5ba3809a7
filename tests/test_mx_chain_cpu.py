"""CPU suite: two forms of the matrix-core top-2 search (bf_mx.hip) that take work out of a wave's serial chain, restated in
numpy on the model of tests/test_mx_ties_cpu.py and driven over chosen schedules; every table is compared with a full sort at
zero tolerance.  Both were measured and neither is in the shipped kernel (DESIGN.md 3c "Chunk starts, the fold's wait, and where
a wave's life goes": the first is slower, the second was not built); this module is the proof that they are EXACT, which is
what a later attempt needs first.

The early chunk start: a chunk of two stages or more draws its worker's NEXT ticket at the start of its second-to-last stage (a chunk
of one stage at the start of that stage, as before), so the next chunk is known throughout the last stage.  A whole last stage
whose successor exists stages the successor's first stage in its shadow and reads bound[] at its own START; the value is
consumed a stage later, at the chunk start, as e = min(e, dist(g) - (row(g) < c0 ? 1 : 0)) with c0 the start of the NEXT chunk,
and the publish test uses the same value.  A bound read earlier is a staler bound - the key of a real row all the same.

Two deliberately wrong forms go through the same checks:
  * rule_current_chunk, the one the change's issue names: the early-read key's row tested against the start of the chunk that
    is ENDING.  A worker's tickets ascend, so that start is below the next chunk's c0, fewer keys count as "below" and ties are
    let in more often, never less: this form is CONSERVATIVE.  It cannot give a wrong table (the issue expected that it would);
    the test asserts the count 0 and that it costs fired groups, which is what it really does.
  * rule_untested: "the key was read while the chunk before was still running, so its row lies below this chunk" - the row is
    not tested and ties are always excluded.  Wrong: a worker that runs ahead publishes from higher chunks between another
    worker's ticket and its early read, and a tie against such a key can win.  The tables show it.
Measured counts are printed by the tests (pytest -s) and stand in DESIGN.md 3c.

The accumulator patch of a group issued ahead of the fold before it: D computed from the old threshold and patched by c_new - c_old in float32 is, bit for bit,
D computed from the new threshold, and a replay that keys group g + 1 from patched values equals the plain replay."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from test_mx_ties_cpu import (GROUP, IDLE, IDX_BITS, IDX_MASK, LIMIT, NO_E, NONE, STAGE, TILE, Model, all_equal,
                              bound_threshold, distances, duplicates, few_values, full_sort, random_rows, rule_always_exclusive)

LLVM = "/opt/rocm/lib/llvm/bin"
OBJDUMP = os.path.join(LLVM, "llvm-objdump")
READELF = os.path.join(LLVM, "llvm-readelf")


def chunk_table(m, two_stage):
    """`two_stage` chunks of two stages, then chunks of one stage to the end: whole ones and, where m is no multiple of the
    stage, a ragged last one - the shape of the planner's tables (uniform chunks, a tail of single stages)."""
    tbl = [0]
    while tbl[-1] < m:
        ln = 2 * STAGE if len(tbl) <= two_stage else STAGE
        tbl.append(min(tbl[-1] + ln, m))
    return tbl


def rule_next_chunk(g, cur_c0, c0):
    return bound_threshold(g, c0)


def rule_current_chunk(g, cur_c0, c0):
    return bound_threshold(g, cur_c0)


def rule_untested(g, cur_c0, c0):
    return rule_always_exclusive(g, c0)


class ChainModel(Model):
    """The model of test_mx_ties_cpu over a chunk TABLE, each worker a generator that yields before every chunk-start exchange
    ("start"), after drawing a ticket a stage early ("drawn") and after every stage ("stage"), so that a schedule can hold a
    worker between its ticket and its early bound read, and between that read and the exchange that consumes it."""

    def __init__(self, d, workers, tbl, early_rule=rule_next_chunk):
        super().__init__(d, workers, strict=True)
        self.tbl = tbl
        self.nchunks = len(tbl) - 1
        self.early_rule = early_rule
        self.published = []                  # (query, key) of every key that reached bound[]
        self.handovers = self.early_reads_of_higher_rows = 0

    def take(self):
        t = self.ticket
        self.ticket += 1
        return t

    def read(self, deliver):
        return {"fresh": self.bound, "stale": self.history[max(0, len(self.history) - 4)], "never": self.history[0]}[deliver].copy()

    def exchange(self, w, g, e_bound):
        _, u2 = self.unite(w)
        pub = (u2 < LIMIT) & (u2 < g)                    # the publish test uses the value that was read; the atomic is a minimum
        for q in np.nonzero(pub)[0]:
            self.published.append((int(q), int(u2[q])))
        self.bound = np.where(pub, np.minimum(self.bound, u2), self.bound)
        self.history.append(self.bound.copy())
        self.e[w] = np.minimum(self.e[w], np.minimum(self.below(u2), e_bound)[:, None])

    def scan(self, w, s0, c1):
        fired = np.zeros(self.nq // TILE, bool)
        for r0 in range(s0, min(s0 + STAGE, c1), GROUP):
            rows = r0 + np.arange(GROUP)
            valid = rows < c1
            dd = np.where(valid[None, :], self.d[:, np.minimum(rows, self.m - 1)], 10**6).reshape(self.nq, 4, 4)
            passing = dd <= self.e[w][:, :, None]
            self.groups += 1
            if not passing.any():
                continue
            self.fired_groups += 1
            tiles = passing.reshape(-1, TILE * 16).any(axis=1)
            fired |= tiles
            sel = np.repeat(tiles, TILE)
            keys = np.where(valid.reshape(1, 4, 4), (dd << IDX_BITS) | rows.reshape(1, 4, 4), NONE)
            allk = np.sort(np.concatenate([self.b1[w][..., None], self.b2[w][..., None], keys], axis=2), axis=2)
            self.b1[w][sel] = allk[sel, :, 0]
            self.b2[w][sel] = allk[sel, :, 1]
            self.e[w][sel] = np.minimum(self.e[w][sel], self.below(self.b2[w][sel]))
        if fired.any():
            _, u2 = self.unite(w)
            sel = np.repeat(fired, TILE)
            self.e[w][sel] = np.minimum(self.e[w][sel], self.below(u2[sel])[:, None])

    def worker(self, w, deliver="fresh"):
        ci, tickets = self.take(), []
        early, cur_c0 = None, 0
        while ci < self.nchunks:
            assert not tickets or ci > tickets[-1]       # a worker's tickets ascend
            tickets.append(ci)
            c0, c1 = self.tbl[ci], self.tbl[ci + 1]
            yield "start"
            if early is None:
                self.exchange(w, self.read(deliver), bound_threshold(self.read(deliver), c0))
            else:
                self.handovers += 1
                real = early < LIMIT
                self.early_reads_of_higher_rows += int(((early[real] & IDX_MASK) >= c0).sum())
                self.exchange(w, early, self.early_rule(early, cur_c0, c0))
            early, cur_c0 = None, c0
            starts = list(range(c0, c1, STAGE))
            nci = None
            for i, s0 in enumerate(starts):
                if i == max(len(starts) - 2, 0):
                    nci = self.take()                    # second-to-last stage, or the only one
                    if len(starts) >= 2:
                        yield "drawn"
                if len(starts) >= 2 and i == len(starts) - 1 and s0 + STAGE == c1 and nci < self.nchunks:
                    early = self.read(deliver)           # the bound for the NEXT chunk start, read at the start of this stage
                self.scan(w, s0, c1)
                yield "stage"
            ci = nci


# ---- schedules ------------------------------------------------------------------------------------------------------------

def step(gen):
    try:
        return next(gen)
    except StopIteration:
        return None


def to_hold(gen):
    """Advance until the worker holds a ticket drawn a stage early, its bound not yet read, or stands in front of a chunk-start
    exchange, its early read (if any) taken."""
    while True:
        s = step(gen)
        if s != "stage":
            return s


def in_turn(mdl, workers, deliver="fresh"):
    gens = [mdl.worker(w, deliver) for w in range(workers)]
    live = list(range(workers))
    while live:
        live = [w for w in live if step(gens[w]) is not None]


def racing(mdl, workers, deliver="fresh", lead=5):
    """Every worker but the last runs to its next hold (to_hold) and stalls there; the last one then runs through `lead` holds,
    publishing from chunks above the tickets the stalled ones hold, before they read or consume their bounds.  Until the queue
    is dry."""
    gens = [mdl.worker(w, deliver) for w in range(workers)]
    live = set(range(workers))
    while live:
        for w in sorted(live - {workers - 1}):
            if to_hold(gens[w]) is None:
                live.discard(w)
        for _ in range(lead):
            if workers - 1 in live and to_hold(gens[workers - 1]) is None:
                live.discard(workers - 1)


def straggler(mdl, workers, deliver="fresh"):
    """Worker 0 takes one step for every eight of each other worker: it holds low chunks while the keys it reads come from rows
    far above them."""
    gens = [mdl.worker(w, deliver) for w in range(workers)]
    live = set(range(workers))
    while live:
        for w in sorted(live):
            for _ in range(1 if w == 0 and len(live) > 1 else 8):
                if w in live and step(gens[w]) is None:
                    live.discard(w)


def stale(mdl, workers):
    in_turn(mdl, workers, "stale")


def never(mdl, workers):
    in_turn(mdl, workers, "never")


def racing_stale(mdl, workers):
    racing(mdl, workers, "stale")


def straggler_stale(mdl, workers):
    straggler(mdl, workers, "stale")


SCHEDULES = [in_turn, racing, straggler, stale, never, racing_stale, straggler_stale]
FAMILIES = [random_rows, few_values, duplicates, all_equal]
# (workers, train rows, two-stage chunks at the head of the table): whole and ragged last stages, one-stage tails, a table of
# two-stage chunks only, and a ragged chunk right behind a chunk of two stages (which no table of the planner has)
SIZES = [(3, 1024, 10), (4, 1000, 9), (1, 512, 8), (7, 909, 8), (2, 640 + 17, 10)]


def cases(early_rule=rule_next_chunk, families=FAMILIES, schedules=SCHEDULES):
    for fam in families:
        for si, (workers, m, two) in enumerate(SIZES):
            rng = np.random.default_rng(1000 + 100 * FAMILIES.index(fam) + si)
            q, t = fam(rng, 2 * TILE, m)
            d = distances(q, t)
            ref = full_sort(d)
            for sched in schedules:
                mdl = ChainModel(d, workers, chunk_table(m, two), early_rule)
                sched(mdl, workers)
                assert mdl.ticket >= mdl.nchunks and mdl.groups == sum((b - a + GROUP - 1) // GROUP for a, b in zip(mdl.tbl, mdl.tbl[1:]))
                yield f"{fam.__name__}/{sched.__name__}/{workers}x{m}", mdl, d, ref


def test_the_tables_have_the_shapes_the_change_touches():
    for workers, m, two in SIZES:
        tbl = chunk_table(m, two)
        lens = [b - a for a, b in zip(tbl, tbl[1:])]
        assert lens[0] == 2 * STAGE and tbl[-1] == m
        if m == 512:
            assert set(lens) == {2 * STAGE}              # the last chunk's successor does not exist
        elif m == 640 + 17:
            assert lens[-2:] == [2 * STAGE, 17]          # a ragged stage handed over by a chunk of two stages
        else:
            assert STAGE in lens[two:]                   # a one-stage tail
        if m % STAGE:
            assert lens[-1] == m % STAGE                 # a ragged last stage


@pytest.mark.parametrize("fam", FAMILIES, ids=lambda f: f.__name__)
@pytest.mark.parametrize("sched", SCHEDULES, ids=lambda f: f.__name__)
def test_early_ticket_and_early_bound_equal_the_full_sort(fam, sched):
    handovers = higher = 0
    for name, mdl, d, ref in cases(families=[fam], schedules=[sched]):
        assert np.array_equal(mdl.result(), ref), name
        # every published key is the key of a real row of its query, at or above the true final 2nd key
        for q, key in mdl.published:
            row = key & IDX_MASK
            assert row < mdl.m and key >> IDX_BITS == d[q, row], name
            assert key >= ref[q, 1], name
        handovers += mdl.handovers
        higher += mdl.early_reads_of_higher_rows
    assert handovers > 0                                 # the path is taken
    if sched in (racing, straggler) and fam in (random_rows, duplicates):
        assert higher > 0                                # and early-read keys do come from rows at or above the chunk they serve


def wrong_tables(rule):
    n = bad = fired = 0
    for name, mdl, d, ref in cases(early_rule=rule, families=[duplicates, few_values]):
        n += 1
        bad += not np.array_equal(mdl.result(), ref)
        fired += mdl.fired_groups
    return n, bad, fired


def test_wrong_rules():
    n, bad0, fired0 = wrong_tables(rule_next_chunk)
    assert bad0 == 0
    # the issue's wrong rule: conservative, see the module docstring
    _, bad_cur, fired_cur = wrong_tables(rule_current_chunk)
    # a rule that is wrong: the early-read key's row not tested at all
    _, bad_un, _ = wrong_tables(rule_untested)
    print(f"tie-heavy cases {n}: wrong tables with the row tested against the current chunk's start {bad_cur} "
          f"(fired groups {fired_cur} against {fired0}), with the row not tested {bad_un}")
    assert bad_cur == 0 and fired_cur >= fired0
    assert bad_un > 0


# ---- the accumulator patch of a group issued ahead ------------------------------------------------------------------------

def c_of(x):
    """The accumulator start for the exclusive threshold x: 2 (x - 1) - 256."""
    return np.float32(2 * int(x) - 258)


def mfma_pair(dot0, dot1, c):
    """Two accumulating steps in float32, as the two K-halves of a group."""
    return (np.asarray(c, np.float32) + dot0.astype(np.float32)).astype(np.float32) + dot1.astype(np.float32)


@pytest.mark.parametrize("fam", [random_rows, few_values], ids=lambda f: f.__name__)
def test_patched_accumulators_are_the_new_threshold_s_bit_for_bit(fam):
    rng = np.random.default_rng(31)
    q, t = fam(rng, TILE, 256)
    pop = np.array([bin(i).count("1") for i in range(256)], np.int64)
    h0 = pop[q[:, None, :16] ^ t[None, :, :16]].sum(-1)
    h1 = pop[q[:, None, 16:] ^ t[None, :, 16:]].sum(-1)
    dot0, dot1 = 128 - 2 * h0, 128 - 2 * h1
    xs = [0, 1, 2, 95, 96, 128, 257, 510, 511]           # x = 0: a threshold of -1; x = 511: the open threshold
    checked = 0
    for x_old in xs:
        for x_new in xs:
            if x_new > x_old:
                continue
            ahead = mfma_pair(dot0, dot1, c_of(x_old))
            patched = (ahead + np.float32(c_of(x_new) - c_of(x_old))).astype(np.float32)
            plain = mfma_pair(dot0, dot1, c_of(x_new))
            assert patched.dtype == np.float32 and np.array_equal(patched.view(np.uint32), plain.view(np.uint32)), (x_old, x_new)
            # and what the update path reads out of it: the pass test and the key's distance
            assert np.array_equal(patched >= 0, (h0 + h1) < x_new)
            dist = (x_new - 1) - (patched.astype(np.int64) >> 1)
            assert np.array_equal(dist, h0 + h1)
            checked += 1
    assert checked == len(xs) * (len(xs) + 1) // 2


def replay(d, ahead, patch=True):
    """One lane's view of one tile, a stage of 8 groups at a time: thresholds per query and lane (x exclusive), keys, the fired
    groups.  ahead: group g + 1's values are computed with the thresholds as they stood BEFORE group g's fold, then patched (or
    not) by the move of the threshold.  Returns (table, fired groups, thresholds after every group)."""
    nq, m = d.shape
    b1 = np.full((nq, 4), NONE, np.int64)
    b2 = b1.copy()
    x = np.full((nq, 4), NO_E, np.int64)
    fired, trace = [], []
    x_issue = x.copy()
    for r0 in range(0, m, GROUP):
        first_of_trip = (r0 // GROUP) % 8 == 0
        xi = x.copy() if (not ahead or first_of_trip) else x_issue      # the thresholds the group's MFMAs started from
        rows = r0 + np.arange(GROUP)
        dd = d[:, rows].reshape(nq, 4, 4)
        dot = 256 - 2 * dd
        D = (2 * xi[:, :, None] - 258 + dot).astype(np.float32)
        if ahead and patch:
            D = (D + (2 * (x - xi))[:, :, None].astype(np.float32)).astype(np.float32)
        x_issue = x.copy()                                              # the next group is issued before this fold
        if (D >= 0).any():
            fired.append(r0 // GROUP)
            dist = (x[:, :, None] - 1) - (D.astype(np.int64) >> 1)     # the key formula reads the CURRENT threshold
            keys = (dist << IDX_BITS) | rows.reshape(1, 4, 4)
            keys = np.where(D >= 0, keys, NONE)                         # rows that do not pass cannot enter (row gates, min / med3)
            allk = np.sort(np.concatenate([b1[..., None], b2[..., None], keys], axis=2), axis=2)
            b1, b2 = allk[..., 0], allk[..., 1]
            x = np.minimum(x, np.where(b2 == NONE, NO_E, b2 >> IDX_BITS))
        trace.append(x.copy())
    k = np.sort(np.concatenate([b1, b2], axis=1), axis=1)[:, :2]
    return k, fired, trace


def test_replay_with_groups_issued_ahead_equals_the_plain_replay():
    wrong = total = 0
    for fi, fam in enumerate([random_rows, few_values, duplicates, all_equal]):
        for seed in range(3):
            rng = np.random.default_rng(50 + 10 * fi + seed)
            q, t = fam(rng, TILE, 384)
            d = distances(q, t)
            plain = replay(d, ahead=False)
            piped = replay(d, ahead=True)
            assert np.array_equal(plain[0], full_sort(d))
            assert np.array_equal(piped[0], plain[0]) and piped[1] == plain[1]
            assert all(np.array_equal(a, b) for a, b in zip(piped[2], plain[2]))
            if fam in (few_values, duplicates):
                total += 1
                wrong += not np.array_equal(replay(d, ahead=True, patch=False)[0], plain[0])
    print(f"without the patch: {wrong} of {total} tie-heavy tables wrong")
    assert wrong > 0


# ---- the built kernel -------------------------------------------------------------------------------------------------------

def test_block_lds_footprint(built, tmp_path):
    if not (os.path.exists(OBJDUMP) and os.path.exists(READELF)):
        pytest.skip("llvm-objdump / llvm-readelf of the ROCm toolchain not found")
    from slamhip import _lib

    tmp = str(tmp_path)
    local = os.path.join(tmp, "lib.so")
    shutil.copy(_lib.LIB_PATH, local)
    subprocess.run([OBJDUMP, "--offloading", local], cwd=tmp, check=True, capture_output=True)
    for f in sorted(os.listdir(tmp)):
        if "gfx950" not in f:
            continue
        notes = subprocess.run([READELF, "--notes", os.path.join(tmp, f)], check=True, capture_output=True, text=True).stdout
        for block in re.split(r"\n\s+- \.agpr_count", notes):
            if re.search(r"\.name:\s+_Z\d+bf_top2_mx_kernel\w*\n", block):
                lds = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", block).group(1))
                assert 32768 <= lds <= 40960, lds
                return
    pytest.fail("bf_top2_mx_kernel is not in the library")
