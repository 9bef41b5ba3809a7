"""CPU suite: the threshold rules of the matrix-core top-2 search (bf_mx.hip, "selection" in its header), restated in numpy
and driven over adversarial schedules; every table is compared with a full sort of the packed keys at zero tolerance.

What is restated: each lane keeps the top-2 of its own rows (four lanes per query, four rows per lane and 16-row group); a
tile of 16 queries takes the update path when one of its pairs is at or below the lane's inclusive threshold e; after a fire
e = min(e, dist(own 2nd) - 1); after a stage that fired e = min(e, dist(2nd of the query's four lanes) - 1); at a chunk start
the worker publishes the 2nd-best KEY of its query into bound[] (only keys below 0x7F000000) and applies the key g it read:
e = min(e, dist(g) - (row(g) < c0 ? 1 : 0)).  Workers draw ascending chunks by ticket.

This module is what pins the rule: which worker reads which bound on a GPU depends on timing, here the schedule is chosen.
test_rule_drops_only_behind_a_smaller_key holds bound_threshold to the correctness argument itself, and the schedules hold
the whole model to the full sort.  Two wrong rules (ties excluded whatever the bound's row; row(g) <= c0) are run through the
same checks in test_wrong_rules_are_caught, so the cases are known to be sharp enough to see them."""
import numpy as np
import pytest

IDX_BITS = 23
IDX_MASK = (1 << IDX_BITS) - 1
NONE = 0xFFFFFFFF
IDLE = 0x7F7F7F7F
LIMIT = 0x7F000000          # bound[] holds keys below this; at or above: nobody has published
NO_E = NONE >> IDX_BITS     # 511: everything passes

GROUP, STAGE, CHUNK = 16, 32, 64      # rows: a small stage (two groups) and chunk (two stages), so that every path is taken often
TILE = 16                             # queries that share one gate

POP = np.array([bin(i).count("1") for i in range(256)], np.int64)


def bound_threshold(g, c0):
    """The inclusive threshold a bound key g read at the start of the chunk beginning at row c0 allows (the shipped rule)."""
    g = np.asarray(g, np.int64)
    return np.where(g < LIMIT, (g >> IDX_BITS) - ((g & IDX_MASK) < c0), NO_E)


def rule_always_exclusive(g, c0):
    g = np.asarray(g, np.int64)
    return np.where(g < LIMIT, (g >> IDX_BITS) - 1, NO_E)


def rule_row_le(g, c0):
    g = np.asarray(g, np.int64)
    return np.where(g < LIMIT, (g >> IDX_BITS) - ((g & IDX_MASK) <= c0), NO_E)


def rule_inclusive(g, c0):
    """The rule before: a bound is a distance, ties pass."""
    g = np.asarray(g, np.int64)
    return np.where(g < LIMIT, g >> IDX_BITS, NO_E)


def distances(q, t):
    return POP[q[:, None, :] ^ t[None, :, :]].sum(-1)


def full_sort(d):
    keys = (d << IDX_BITS) | np.arange(d.shape[1], dtype=np.int64)[None, :]
    k = np.sort(keys, axis=1)[:, :2]
    if k.shape[1] < 2:
        k = np.concatenate([k, np.full((len(k), 2 - k.shape[1]), NONE, np.int64)], axis=1)
    return k


class Model:
    """W workers over the chunks of M rows; strict = the exclusive thresholds of this kernel, else the inclusive ones of before."""

    def __init__(self, d, workers, strict=True, rule=None):
        self.d = d
        self.nq, self.m = d.shape
        assert self.nq % TILE == 0
        self.strict = strict
        self.rule = rule if rule is not None else (bound_threshold if strict else rule_inclusive)
        self.b1 = np.full((workers, self.nq, 4), NONE, np.int64)
        self.b2 = self.b1.copy()
        self.e = np.full((workers, self.nq, 4), NO_E, np.int64)
        self.bound = np.full(self.nq, IDLE, np.int64)
        self.history = [self.bound.copy()]
        self.ticket = 0
        self.nchunks = (self.m + CHUNK - 1) // CHUNK
        self.drawn = [None] * workers
        self.groups = self.fired_groups = 0

    def below(self, key):
        """The threshold a known 2nd-best key from rows below every row still to come allows."""
        return np.where(key == NONE, NO_E, (key >> IDX_BITS) - (1 if self.strict else 0))

    def unite(self, w):
        k = np.sort(np.concatenate([self.b1[w], self.b2[w]], axis=1), axis=1)
        return k[:, 0], k[:, 1]

    def draw(self, w):
        assert self.drawn[w] is None
        if self.ticket < self.nchunks:
            self.drawn[w] = self.ticket
        self.ticket += 1
        return self.drawn[w] is not None

    def run(self, w, deliver="fresh"):
        """Exchange at the start of the drawn chunk, then its scan.  deliver: fresh, stale (bound[] as it was three exchanges ago), never (bound[] idle)."""
        c = self.drawn[w]
        self.drawn[w] = None
        c0, c1 = c * CHUNK, min((c + 1) * CHUNK, self.m)
        _, u2 = self.unite(w)
        g = {"fresh": self.bound, "stale": self.history[max(0, len(self.history) - 4)], "never": self.history[0]}[deliver].copy()
        pub = (u2 < LIMIT) & (u2 < self.bound)
        self.bound = np.where(pub, u2, self.bound)
        self.history.append(self.bound.copy())
        self.e[w] = np.minimum(self.e[w], np.minimum(self.below(u2), self.rule(g, c0))[:, None])
        for s0 in range(c0, c1, STAGE):
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

    def result(self):
        k = np.concatenate([self.b1.transpose(1, 0, 2).reshape(self.nq, -1), self.b2.transpose(1, 0, 2).reshape(self.nq, -1)], axis=1)
        return np.sort(k, axis=1)[:, :2]


# ---- schedules: each drives a Model to the end of the queue -------------------------------------------------------------

def in_turn(mdl, workers, deliver="fresh"):
    live = True
    while live:
        live = False
        for w in range(workers):
            if mdl.draw(w):
                mdl.run(w, deliver)
                live = True


def racing(mdl, workers, deliver="fresh", lead=5):
    """Every worker but the last draws a chunk and stalls in front of its exchange; the last one then runs `lead` chunks - and
    publishes from them - before the stalled ones read the bound for their LOWER chunks.  Repeated until the queue is dry."""
    while True:
        held = [w for w in range(workers - 1) if mdl.draw(w)]
        for _ in range(lead):
            if mdl.draw(workers - 1):
                mdl.run(workers - 1, deliver)
        for w in held:
            mdl.run(w, deliver)
        if mdl.ticket >= mdl.nchunks + workers:
            break


def stale(mdl, workers):
    in_turn(mdl, workers, "stale")


def never(mdl, workers):
    in_turn(mdl, workers, "never")


def racing_stale(mdl, workers):
    racing(mdl, workers, "stale")


SCHEDULES = [in_turn, racing, stale, never, racing_stale]


# ---- data ----------------------------------------------------------------------------------------------------------------

def random_rows(rng, nq, m):
    return rng.integers(0, 256, (nq, 32), dtype=np.uint8), rng.integers(0, 256, (m, 32), dtype=np.uint8)


def few_values(rng, nq, m):
    """Rows drawn from two byte values in a few positions: dozens of rows tie at d1 and d2."""
    vals = np.array([0x00, 0x0F], np.uint8)
    q, t = np.zeros((nq, 32), np.uint8), np.zeros((m, 32), np.uint8)
    q[:, :3] = vals[rng.integers(0, 2, (nq, 3))]
    t[:, :3] = vals[rng.integers(0, 2, (m, 3))]
    return q, t


def duplicates(rng, nq, m):
    """Each query's nearest rows are exact copies of one vector placed in low, middle and high chunks."""
    q, t = random_rows(rng, nq, m)
    for i in range(nq):
        v = q[i].copy()
        v[rng.integers(0, 32)] ^= 1 << rng.integers(0, 8)
        for lo, hi in ((0, m // 4), (m // 4, m // 2), (m // 2, m)):
            t[rng.integers(lo, hi)] = v
        t[rng.integers(0, m, 3)] = v
    return q, t


def all_equal(rng, nq, m):
    v = rng.integers(0, 256, 32, dtype=np.uint8)
    return np.tile(v, (nq, 1)), np.tile(v, (m, 1))


FAMILIES = [random_rows, few_values, duplicates, all_equal]
SIZES = [(3, 1024), (4, 1000), (1, 512), (7, 909)]      # (workers, train rows): whole and ragged last chunks


def tables(rule=None, strict=True, families=FAMILIES, schedules=SCHEDULES):
    """(case name, model table, full sort) of every family x schedule x size."""
    for fam in families:
        for si, (workers, m) in enumerate(SIZES):
            rng = np.random.default_rng(100 * FAMILIES.index(fam) + si)
            q, t = fam(rng, 2 * TILE, m)
            d = distances(q, t)
            ref = full_sort(d)
            for sched in schedules:
                mdl = Model(d, workers, strict, rule)
                sched(mdl, workers)
                yield f"{fam.__name__}/{sched.__name__}/{workers}x{m}", mdl.result(), ref


@pytest.mark.parametrize("fam", FAMILIES, ids=lambda f: f.__name__)
@pytest.mark.parametrize("sched", SCHEDULES, ids=lambda f: f.__name__)
def test_exclusive_thresholds_equal_the_full_sort(fam, sched):
    for name, got, ref in tables(families=[fam], schedules=[sched]):
        assert np.array_equal(got, ref), name


@pytest.mark.parametrize("sched", SCHEDULES, ids=lambda f: f.__name__)
def test_inclusive_thresholds_equal_the_full_sort(sched):
    """The model with the rule of before is the same search: the comparison below is between two right answers."""
    for name, got, ref in tables(strict=False, schedules=[sched]):
        assert np.array_equal(got, ref), name


def rule_faults(rule):
    """Cases in which `rule` drops a candidate that no smaller key stands in front of.  A bound key K read at the start of the
    chunk at c0 may drop the candidate (dist, row), row >= c0, only if K < (dist << 23 | row) - K itself included: a key does
    not stand in front of itself - and K is not below the limit only when nobody has published."""
    faults = []
    for c0 in (0, 64, 128):
        for grow in (0, c0 - 1, c0, c0 + 1, c0 + 63, c0 + 200):
            if grow < 0:
                continue
            for gd in (0, 1, 95, 253):
                g = (gd << IDX_BITS) | grow
                e = int(rule(g, c0))
                for row in (c0, c0 + 1, c0 + 63):
                    for dist in range(0, 257):
                        if dist > e and not g < ((dist << IDX_BITS) | row):
                            faults.append((c0, gd, grow, dist, row))
    for g in (LIMIT, IDLE, NONE):
        if int(rule(g, 64)) < 256:
            faults.append(("idle", g))
    return faults


def test_rule_drops_only_behind_a_smaller_key():
    assert rule_faults(bound_threshold) == []
    # and it is not vacuous: a bound from below the chunk does exclude its ties, one from inside or above does not
    assert int(bound_threshold((95 << IDX_BITS) | 63, 64)) == 94
    assert int(bound_threshold((95 << IDX_BITS) | 64, 64)) == 95
    assert int(bound_threshold((95 << IDX_BITS) | 700, 64)) == 95
    assert int(bound_threshold(IDLE, 64)) == NO_E


def test_exclusive_rule_fires_fewer_groups_on_random_rows():
    """What the rule is for.  Random 256-bit rows, workers in turn: the same table from strictly fewer fired groups."""
    rng = np.random.default_rng(7)
    q, t = random_rows(rng, 4 * TILE, 4096)
    d = distances(q, t)
    fired = {}
    for strict in (False, True):
        mdl = Model(d, 4, strict)
        in_turn(mdl, 4)
        assert np.array_equal(mdl.result(), full_sort(d))
        fired[strict] = mdl.fired_groups
        assert mdl.groups == 4096 // GROUP
    print("fired groups of", 4096 // GROUP, ": inclusive", fired[False], "exclusive", fired[True])
    assert fired[True] < fired[False]


@pytest.mark.parametrize("wrong", [rule_always_exclusive, rule_row_le], ids=lambda f: f.__name__)
def test_wrong_rules_are_caught(wrong):
    """The two wrong rules of the header, through the same checks: each must fail at least one of them."""
    by_argument = len(rule_faults(wrong))
    by_tables = sum(not np.array_equal(got, ref) for _, got, ref in tables(rule=wrong, families=[duplicates, few_values]))
    print(wrong.__name__, ": faults against the argument", by_argument, ", wrong tables", by_tables)
    assert by_argument > 0
    if wrong is rule_always_exclusive:
        assert by_tables > 0        # reachable: a racing worker's bound carries a higher row at the same distance
