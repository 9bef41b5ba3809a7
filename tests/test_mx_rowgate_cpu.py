"""CPU suite: the row gates of the matrix-core top-2 search (bf_mx.hip, "row gates" in its header), restated in numpy on top
of tests/test_mx_head_cpu.py (whose model, chunk tables and schedules are imported, with the rules, data families and full
sort of tests/test_mx_ties_cpu.py) and compared with a full sort of the packed keys at zero tolerance.

What is restated on top of those modules: in a tile that takes the update path, a lane's row r (of its four rows of the
16-row group) enters the lane's pair only if SOME lane of the tile passes at r - one wave-uniform test per row in the
kernel; the rows of an open gate enter in every lane of the tile, passing or not.  A skipped row has a distance above the
threshold in every lane, so by the threshold rules it is not in the final top-2 - the argument that lets a group that
does not fire skip all of its rows.  Fewer losing rows enter a lane's pair, so its 2nd-best key, the thresholds and the
published keys can be LARGER than without the gates; they stay keys of real rows, hence valid bounds.  The suite asserts
both halves: equal tables, and every published key a real row's key that is at least the query's true final 2nd key.

A wrong gate goes through the same checks in test_wrong_gate_is_caught: the row gate opening on D > 0 in place of D >= 0
(distance below e in place of at or below e) while the tile's gate stays as it is - a tile fires for a row AT the
threshold, which then never enters."""
import numpy as np
import pytest

from test_mx_head_cpu import SCHEDULES, SIZES, HeadModel, in_turn, table
from test_mx_ties_cpu import (FAMILIES, GROUP, IDX_BITS, LIMIT, NONE, TILE, all_equal, distances, duplicates, few_values, full_sort,
                              random_rows)


def gate_at_or_below(dd, e):
    """The shipped gate: D >= 0, the row is at or below the lane's inclusive threshold."""
    return dd <= e


def gate_below(dd, e):
    """The wrong gate: D > 0."""
    return dd < e


class RowGateModel(HeadModel):
    """HeadModel with the update of a fired tile gated per row; gate(dd, e) says which lanes pass at a row."""

    def __init__(self, *args, gate=gate_at_or_below, **kw):
        super().__init__(*args, **kw)
        self.gate = gate
        self.rows_open = self.rows_of_fired_tiles = 0
        self.published = []                      # (query, key) of every key a worker put into bound[]

    def exchange(self, w, row, deliver):
        before = self.bound.copy()
        super().exchange(w, row, deliver)
        for qi in np.nonzero(self.bound != before)[0]:
            self.published.append((int(qi), int(self.bound[qi])))

    def scan(self, w, s0, s1, c1):
        fired = np.zeros(self.nq // TILE, bool)
        for r0 in range(s0, s1, GROUP):
            rows = r0 + np.arange(GROUP)
            valid = rows < c1
            dd = np.where(valid[None, :], self.d[:, np.minimum(rows, self.m - 1)], 10**6).reshape(self.nq, 4, 4)   # [query, kg, r]
            e = self.e[w][:, :, None]
            passing = dd <= e
            self.groups += 1
            if not passing.any():
                continue
            self.fired_groups += 1
            tiles = passing.reshape(-1, TILE * 16).any(axis=1)
            fired |= tiles
            self.fired_tiles += int(tiles.sum())
            # the row gates: per tile and r, some lane (16 queries x 4 quarters) passes the gate's own test
            open_ = self.gate(dd, e).reshape(-1, TILE, 4, 4).any(axis=(1, 2)) & tiles[:, None]                  # [tile, r]
            self.rows_open += int(open_.sum())
            self.rows_of_fired_tiles += 4 * int(tiles.sum())
            enter = np.repeat(open_, TILE, axis=0)[:, None, :] & valid.reshape(1, 4, 4)
            keys = np.where(enter, (dd << IDX_BITS) | rows.reshape(1, 4, 4), NONE)
            allk = np.sort(np.concatenate([self.b1[w][..., None], self.b2[w][..., None], keys], axis=2), axis=2)
            sel = np.repeat(tiles, TILE)
            self.b1[w][sel] = allk[sel, :, 0]
            self.b2[w][sel] = allk[sel, :, 1]
            self.e[w][sel] = np.minimum(self.e[w][sel], self.below(self.b2[w][sel]))
        if fired.any():
            _, u2 = self.unite(w)
            sel = np.repeat(fired, TILE)
            self.e[w][sel] = np.minimum(self.e[w][sel], self.below(u2[sel])[:, None])


def tables(gate=gate_at_or_below, families=FAMILIES, schedules=SCHEDULES, sizes=SIZES):
    """(case name, model, distances, full sort) of every family x size x schedule, on the seeds of test_mx_head_cpu."""
    for fam in families:
        for si, (workers, m, chunk) in enumerate(sizes):
            rng = np.random.default_rng(1000 + 100 * FAMILIES.index(fam) + si)
            q, t = fam(rng, 2 * TILE, m)
            d = distances(q, t)
            ref = full_sort(d)
            for sched in schedules:
                mdl = RowGateModel(d, workers, table(m, chunk, workers), gate=gate)
                sched(mdl, workers)
                assert mdl.groups == sum(-(-(b - a) // GROUP) for a, b in zip(mdl.tbl, mdl.tbl[1:])), "a chunk was not scanned"
                yield f"{fam.__name__}/{sched.__name__}/{workers}x{m}/{chunk}", mdl, d, ref


def bad_published_keys(mdl, d, ref):
    """Published keys that are not a real row's key of that query, or lie below the query's true final 2nd key."""
    bad = []
    for qi, key in mdl.published:
        row, dist = key & ((1 << IDX_BITS) - 1), key >> IDX_BITS
        if not (key < LIMIT and row < mdl.m and d[qi, row] == dist and key >= ref[qi, 1]):
            bad.append((qi, key))
    return bad


@pytest.mark.parametrize("fam", FAMILIES, ids=lambda f: f.__name__)
@pytest.mark.parametrize("sched", SCHEDULES, ids=lambda f: f.__name__)
def test_row_gates_equal_the_full_sort_and_publish_valid_bounds(fam, sched):
    published = 0
    for name, mdl, d, ref in tables(families=[fam], schedules=[sched]):
        assert np.array_equal(mdl.result(), ref), name
        assert bad_published_keys(mdl, d, ref) == [], name
        published += len(mdl.published)
    assert published > 0


@pytest.mark.parametrize("seed", [11, 12, 13])
def test_gates_skip_rows_and_leave_the_search_as_it_was(seed):
    """What the gates are for: on random rows most rows of an updated tile stay out, and the tiles that fire are the same
    count or more only by what larger thresholds allow - the tables are equal either way."""
    rng = np.random.default_rng(seed)
    d = distances(*random_rows(rng, 4 * TILE, 4096))
    plain = HeadModel(d, 4, table(4096, 256, 4))
    in_turn(plain, 4)
    gated = RowGateModel(d, 4, table(4096, 256, 4))
    in_turn(gated, 4)
    assert np.array_equal(gated.result(), full_sort(d)) and np.array_equal(plain.result(), full_sort(d))
    print("tile updates: plain", plain.fired_tiles, ", gated", gated.fired_tiles, "; rows of updated tiles that enter:",
          gated.rows_open, "of", gated.rows_of_fired_tiles)
    assert 0 < gated.rows_open < gated.rows_of_fired_tiles // 2
    # larger thresholds can only let more through, never fewer
    assert gated.fired_tiles >= plain.fired_tiles


def test_all_equal_rows_open_no_gate_after_the_first_two():
    """Every row ties: only the first group fires (every threshold is still open there); after it no gate opens."""
    rng = np.random.default_rng(3)
    d = distances(*all_equal(rng, 2 * TILE, 1024))
    mdl = RowGateModel(d, 1, table(1024, 256, 1))
    in_turn(mdl, 1)
    assert np.array_equal(mdl.result(), full_sort(d))
    assert mdl.fired_groups == 1 and mdl.rows_open == 4 * (2 * TILE // TILE)     # the first group: all four rows of each tile tie at 0


def test_wrong_gate_is_caught():
    """The gate on D > 0 through the same checks, on the tie-heavy families; the count is printed."""
    wrong = [name for name, mdl, d, ref in tables(gate=gate_below, families=[few_values, duplicates, all_equal])
             if not np.array_equal(mdl.result(), ref)]
    print("row gate on D > 0: wrong tables", len(wrong), "of", 3 * len(SIZES) * len(SCHEDULES), wrong[:3])
    assert len(wrong) > 0
