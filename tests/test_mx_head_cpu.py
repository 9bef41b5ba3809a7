"""CPU suite: the early bound exchanges of the matrix-core top-2 search (bf_mx.hip, SLAM_MX_EARLY), restated in numpy in the
manner of tests/test_mx_ties_cpu.py (whose constants, rules, data families and full sort are imported) and driven over
chosen schedules; every table is compared with a full sort of the packed keys at zero tolerance.

What is restated on top of that module: a worker counts the rows it has scanned since launch, and after a stage at whose
end the count is one of the early points - unless the stage is the last of its chunk - it runs the exchange of a chunk
start before the next stage: it publishes the 2nd-best KEY of its query and applies the key g it read with
e = min(e, dist(g) - (row(g) < s1 ? 1 : 0)), s1 = the first row of the stage to come, the first row the lane has still to
see.  Chunks come from a boundary table (uniform chunks first, shrinking ones last, a ragged end); workers draw them by
ticket, and a worker can be held in front of any exchange, at a chunk start or at an early point.

Two wrong rules go through the same checks in test_wrong_rules_are_caught:
  * ties always excluded on a foreign key: it drops rows that win their tie on the index - wrong tables on the racing
    schedules, and faults against the argument;
  * the foreign key's row tested against the CHUNK start c0 in place of the stage start s1: c0 <= s1, so this rule keeps
    every tie the right rule keeps and more.  It cannot drop a row that belongs in the table, and no schedule gives a
    wrong table with it (the test asserts that too: it is why a GPU run of such a build agrees with the VALU kernel).
    As a rule it is caught by the other half of the contract, that the threshold is the LOWEST one the argument allows
    (rule_slack).  In the search it changes nothing at all: rows c0 .. s1 - 1 are scanned by this worker alone, so a key
    from there is one this worker published, its own united 2nd-best key is at or below it, and that key excludes the
    ties anyway.  The test asserts the equal count of tile updates, so that nobody takes the slack for a cost."""
import numpy as np
import pytest

from test_mx_ties_cpu import (FAMILIES, GROUP, IDLE, IDX_BITS, IDX_MASK, LIMIT, NO_E, NONE, TILE, all_equal, bound_threshold,
                              distances, duplicates, few_values, full_sort, random_rows, rule_always_exclusive)

STAGE = 32                      # rows: two groups
EARLY = (32, 64, 128)           # rows scanned: after 1, 2 and 4 stages, as 128, 256 and 512 rows are with the 128-row stage


def table(m, chunk, workers):
    """Chunk boundaries in the planner's manner: uniform chunks, then (rest / 2 workers) rounded down to whole stages, never
    below one stage; the last chunk ends at m, ragged or not."""
    b, at = [0], 0
    while at < m:
        g = (m - at) // (2 * workers) // STAGE * STAGE
        at = min(m, at + (chunk if g >= chunk else max(g, STAGE)))
        b.append(at)
    return b


class HeadModel:
    """W workers over a chunk table.  first_row: what the early exchange hands the rule - "stage" (the shipped choice: the
    first row of the stage to come) or "chunk" (the chunk's first row, the wrong build)."""

    def __init__(self, d, workers, tbl, early=EARLY, rule=bound_threshold, first_row="stage"):
        self.d = d
        self.nq, self.m = d.shape
        assert self.nq % TILE == 0 and tbl[0] == 0 and tbl[-1] == self.m
        self.tbl, self.early, self.rule, self.first_row = tbl, set(early), rule, first_row
        self.b1 = np.full((workers, self.nq, 4), NONE, np.int64)
        self.b2 = self.b1.copy()
        self.e = np.full((workers, self.nq, 4), NO_E, np.int64)
        self.bound = np.full(self.nq, IDLE, np.int64)
        self.history = [self.bound.copy()]
        self.ticket = 0
        self.scanned = [0] * workers
        self.groups = self.fired_groups = self.fired_tiles = self.early_exchanges = 0

    @staticmethod
    def below(key):
        """The threshold a known 2nd-best key from rows below every row still to come allows."""
        return np.where(key == NONE, NO_E, (key >> IDX_BITS) - 1)

    def unite(self, w):
        k = np.sort(np.concatenate([self.b1[w], self.b2[w]], axis=1), axis=1)
        return k[:, 0], k[:, 1]

    def exchange(self, w, row, deliver):
        """Publish the worker's 2nd-best key, apply the key read; row = what the rule takes for the first row still to come."""
        _, u2 = self.unite(w)
        g = {"fresh": self.bound, "stale": self.history[max(0, len(self.history) - 4)], "never": self.history[0]}[deliver].copy()
        pub = (u2 < LIMIT) & (u2 < self.bound)
        self.bound = np.where(pub, u2, self.bound)
        self.history.append(self.bound.copy())
        self.e[w] = np.minimum(self.e[w], np.minimum(self.below(u2), self.rule(g, row))[:, None])

    def scan(self, w, s0, s1, c1):
        fired = np.zeros(self.nq // TILE, bool)
        for r0 in range(s0, s1, GROUP):
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
            self.fired_tiles += int(tiles.sum())
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
        """A generator: the worker's life, yielding in front of every exchange - the ticket of a chunk is drawn before."""
        while True:
            c = self.ticket
            self.ticket += 1
            if c >= len(self.tbl) - 1:
                return
            c0, c1 = self.tbl[c], self.tbl[c + 1]
            yield "chunk"
            self.exchange(w, c0, deliver)
            for s0 in range(c0, c1, STAGE):
                s1 = s0 + STAGE
                self.scan(w, s0, min(s1, c1), c1)
                self.scanned[w] += min(s1, c1) - s0
                if s1 < c1 and self.scanned[w] in self.early:
                    yield "early"
                    self.early_exchanges += 1
                    self.exchange(w, s1 if self.first_row == "stage" else c0, deliver)

    def result(self):
        k = np.concatenate([self.b1.transpose(1, 0, 2).reshape(self.nq, -1), self.b2.transpose(1, 0, 2).reshape(self.nq, -1)], axis=1)
        return np.sort(k, axis=1)[:, :2]


# ---- schedules: each drives every worker of a HeadModel to the end of the queue ----------------------------------------------

def step(gens, w):
    """Run worker w up to its next exchange; False once it has run dry."""
    if gens[w] is None:
        return False
    try:
        next(gens[w])
        return True
    except StopIteration:
        gens[w] = None
        return False


def in_turn(mdl, workers, deliver="fresh"):
    """Workers in step, one exchange each in turn: what blocks that start together do."""
    gens = [mdl.worker(w, deliver) for w in range(workers)]
    while any([step(gens, w) for w in range(workers)]):
        pass


def racing(mdl, workers, deliver="fresh", lead=9):
    """Every worker but the last runs up to its next exchange - at a chunk start or at an early point - and is held in front
    of it; the last one then passes `lead` exchanges, publishing from higher rows, before the held ones read."""
    gens = [mdl.worker(w, deliver) for w in range(workers)]
    live = True
    while live:
        live = False
        for _ in range(lead):
            live |= step(gens, workers - 1)
        for w in range(workers - 1):
            live |= step(gens, w)


def straggler(mdl, workers, deliver="fresh"):
    """Worker 0 draws the first chunk and is held in front of EVERY exchange until all the others have run dry: each of its
    early exchanges reads keys from far higher rows."""
    gens = [mdl.worker(w, deliver) for w in range(workers)]
    step(gens, 0)
    while any([step(gens, w) for w in range(1, workers)]):
        pass
    while step(gens, 0):
        pass


def stale(mdl, workers):
    in_turn(mdl, workers, "stale")


def never(mdl, workers):
    in_turn(mdl, workers, "never")


def racing_stale(mdl, workers):
    racing(mdl, workers, "stale")


SCHEDULES = [in_turn, racing, straggler, stale, never, racing_stale]

# (workers, train rows, uniform chunk rows): 8 stages per chunk with all three early points inside the first chunk, as
# 1024-row chunks have them; 2 stages per chunk, where only the first point falls inside a chunk, as with 256-row chunks;
# one worker; a train set that ends inside the first chunk with a ragged last stage
SIZES = [(3, 2048, 256), (2, 1500, 256), (4, 1000, 64), (1, 700, 256), (2, 90, 256), (7, 909, 64)]


def tables(rule=bound_threshold, first_row="stage", families=FAMILIES, schedules=SCHEDULES, sizes=SIZES):
    """(case name, model, full sort) of every family x size x schedule."""
    for fam in families:
        for si, (workers, m, chunk) in enumerate(sizes):
            rng = np.random.default_rng(1000 + 100 * FAMILIES.index(fam) + si)
            q, t = fam(rng, 2 * TILE, m)
            d = distances(q, t)
            ref = full_sort(d)
            for sched in schedules:
                mdl = HeadModel(d, workers, table(m, chunk, workers), rule=rule, first_row=first_row)
                sched(mdl, workers)
                assert mdl.groups == sum(-(-(b - a) // GROUP) for a, b in zip(mdl.tbl, mdl.tbl[1:])), "a chunk was not scanned"
                yield f"{fam.__name__}/{sched.__name__}/{workers}x{m}/{chunk}", mdl, ref


def test_table_has_uniform_chunks_first_and_a_ragged_end():
    assert table(2048, 256, 3)[:4] == [0, 256, 512, 768] and table(2048, 256, 3)[-1] == 2048
    b = table(1500, 256, 2)
    lens = np.diff(b)
    assert lens[0] == 256 and (np.diff(lens[:-1]) <= 0).all() and lens[-1] % STAGE != 0 and (lens[:-1] % STAGE == 0).all()
    assert table(90, 256, 2) == [0, 32, 64, 90]


@pytest.mark.parametrize("fam", FAMILIES, ids=lambda f: f.__name__)
@pytest.mark.parametrize("sched", SCHEDULES, ids=lambda f: f.__name__)
def test_early_exchanges_equal_the_full_sort(fam, sched):
    early = 0
    for name, mdl, ref in tables(families=[fam], schedules=[sched]):
        assert np.array_equal(mdl.result(), ref), name
        early += mdl.early_exchanges
    assert early > 0


def test_early_points_fall_where_the_kernel_has_them():
    """All three points inside a first chunk of 8 stages; only the first inside a chunk of 2 stages (the other counts fall on
    chunk starts, which exchange anyway, once); none when the chunks are single stages."""
    d = distances(*random_rows(np.random.default_rng(3), TILE, 2048))
    for workers, chunk, want in ((1, 256, 3), (4, 256, 12), (1, 64, 1), (4, 64, 4), (1, STAGE, 0)):
        mdl = HeadModel(d, workers, table(2048, chunk, workers) if chunk > STAGE else list(range(0, 2049, STAGE)))
        in_turn(mdl, workers)
        assert mdl.early_exchanges == want, (workers, chunk)
        assert np.array_equal(mdl.result(), full_sort(d))


# ---- the rule itself ---------------------------------------------------------------------------------------------------------

def rule_cases():
    """(chunk start c0, first row still to come s1, bound key g) over rows of g below, at and above both."""
    for c0 in (0, 256, 1024):
        for s1 in (c0 + STAGE, c0 + 2 * STAGE, c0 + 4 * STAGE):
            for grow in (0, c0 - 1, c0, c0 + 1, s1 - 1, s1, s1 + 1, s1 + 700):
                if grow >= 0:
                    for gd in (0, 1, 95, 253):
                        yield c0, s1, (gd << IDX_BITS) | grow


def rule_faults(rule, first_row):
    """Soundness: a key K read before the scan of rows >= s1 may drop the candidate (dist, row) only if K < (dist << 23 | row).
    first_row(c0, s1) is the row the exchange hands the rule."""
    faults = []
    for c0, s1, g in rule_cases():
        e = int(rule(g, first_row(c0, s1)))
        for row in (s1, s1 + 1, s1 + 63):
            faults += [(c0, s1, g, dist, row) for dist in range(e + 1, 257) if not g < ((dist << IDX_BITS) | row)]
    return faults


def rule_slack(rule, first_row):
    """Tightness: the threshold is the lowest sound one.  Lowering it by one must drop some candidate that no smaller key
    stands in front of (or the threshold is -1 already)."""
    slack = []
    for c0, s1, g in rule_cases():
        e = int(rule(g, first_row(c0, s1)))
        if e >= 0 and all(g < ((e << IDX_BITS) | row) for row in (s1, s1 + 1, s1 + 63, (1 << IDX_BITS) - 1)):
            slack.append((c0, s1, g, e))
    return slack


def stage_start(c0, s1):
    return s1


def chunk_start(c0, s1):
    return c0


def test_rule_is_sound_and_as_low_as_the_argument_allows():
    assert rule_faults(bound_threshold, stage_start) == []
    assert rule_slack(bound_threshold, stage_start) == []
    # not vacuous: a key from the scanned part of the worker's own chunk excludes its ties, one from the stage to come does not
    c0, s1 = 256, 256 + 2 * STAGE
    assert int(bound_threshold((95 << IDX_BITS) | (c0 + 5), s1)) == 94
    assert int(bound_threshold((95 << IDX_BITS) | (s1 - 1), s1)) == 94
    assert int(bound_threshold((95 << IDX_BITS) | s1, s1)) == 95
    assert int(bound_threshold(IDLE, s1)) == NO_E


def fired_on_ties(first_row):
    """Tile updates over tie-heavy rows, workers in step, summed over the sizes with early points."""
    return sum(mdl.fired_tiles for _, mdl, _ in tables(first_row=first_row, families=[few_values, all_equal], schedules=[in_turn],
                                                      sizes=SIZES[:3]))


def test_wrong_rules_are_caught():
    """Each wrong rule of the header through the same checks; the figures are printed."""
    # ties always excluded on a foreign key: unsound, and the schedules reach it
    faults = len(rule_faults(rule_always_exclusive, stage_start))
    wrong = [name for name, mdl, ref in tables(rule=rule_always_exclusive, families=[duplicates, few_values])
             if not np.array_equal(mdl.result(), ref)]
    print("always exclusive: faults against the argument", faults, ", wrong tables", len(wrong), wrong[:3])
    assert faults > 0 and len(wrong) > 0
    # the chunk start in place of the stage start: sound, every table right, slack as a rule - and the same search (header)
    faults = len(rule_faults(bound_threshold, chunk_start))
    slack = len(rule_slack(bound_threshold, chunk_start))
    wrong = [name for name, mdl, ref in tables(first_row="chunk", families=[duplicates, few_values])
             if not np.array_equal(mdl.result(), ref)]
    fired = {f: fired_on_ties(f) for f in ("stage", "chunk")}
    print("chunk start: faults", faults, ", slack cases", slack, ", wrong tables", len(wrong), ", tile updates", fired)
    assert faults == 0 and wrong == []
    assert slack > 0
    assert fired["chunk"] == fired["stage"] > 0


def test_early_exchanges_fire_fewer_groups_on_random_rows():
    """What the exchanges are for.  Random 256-bit rows, four workers in step: the same table from fewer tile updates."""
    rng = np.random.default_rng(11)
    d = distances(*random_rows(rng, 4 * TILE, 4096))
    fired = {}
    for early in ((), EARLY):
        mdl = HeadModel(d, 4, table(4096, 256, 4), early=early)
        in_turn(mdl, 4)
        assert np.array_equal(mdl.result(), full_sort(d))
        fired[early] = mdl.fired_tiles
    print("tile updates of", 4 * 4096 // GROUP, ": chunk starts only", fired[()], ", with early exchanges", fired[EARLY])
    assert fired[EARLY] < fired[()]
