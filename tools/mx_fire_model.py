"""The threshold schedule of the matrix-core top-2 searches (bf_mx.hip, bf_mx32.hip) restated in numpy: how many tile-groups
take the update path, how many row gates open, how many unions and exchanges run (development aid; no GPU, no library).

    python tools/mx_fire_model.py                 # the six rows of DESIGN.md 3c "The stage tail" (about a minute)
    python tools/mx_fire_model.py --tile 32 --union off --workers 4 [--n 256] [--m 65536] [--seed-q 228] [--seed-t 229]
    python tools/mx_fire_model.py --tile 16 --union on --plan-n 65536 --cus 256      # workers and table as planned for that N

What is restated, for one query block (--n queries, a multiple of 64; the first rows of the benchmark's generator):
  * the plan (make_mx_plan_core of bf_mx.hip): the chunk boundary table and the worker count of a shape;
  * tickets: a worker draws its first chunk at launch and the next one at the start of its chunk's last stage; `equal_rate`
    advances every worker by one stage per round, in worker order (on a GPU the order is a matter of timing: the tests drive the
    same model through racing, stale and never-delivered schedules);
  * a lane's state: per query `lanes` lanes (2 in the 32x32 kernel, 4 in the 16x16 one), each with the top-2 keys of ITS rows and
    the exclusive threshold x; lane l of the 32x32 kernel holds rows 8 (k >> 2) + 4 l + (k & 3), k = 0 .. 15, of a 32-row group,
    lane l of the 16x16 kernel rows 4 l + k, k = 0 .. 3, of a 16-row group;
  * a fold: the tile (32 or 16 queries) fires when some row of some lane is below that lane's x - in the 32x32 kernel also
    whenever x > 129, where its compare pattern is INT_MIN; the row gates (a row is keyed and merged in ALL lanes of a fired tile
    when it passes in one) are taken against the thresholds as they stood before the fold; umed3 / min; x = min(x, dist(own
    2nd-best));
  * the stage end: with `union`, x = min(x, dist(2nd-best of the query's lanes)) in the tiles that fired in the stage; the early
    exchanges (SLAM_MX_EARLY) and the chunk-start exchange: unite, publish the united 2nd-best key below the limit, read
    bound[], x = min(x, mx_bound_x(g, first row to come), dist(united 2nd-best));
  * `carry` (32x32 geometry): the fold of a wave's tile 1 (the odd tiles) in the last group of a whole stage that another stage
    of the chunk follows runs AFTER that stage's end instead of in front of it: "whole" carries only where no early exchange
    stands at the stage end (the form DESIGN.md describes and the kernel does not take), "across_exchange" carries there too
    (wrong: the exchange sets x for rows at or above the next stage's first row, the carried rows are below it).
Not restated: rows past the end of a short stage never open a gate here (in the kernels they can, and their keys are dropped)."""
import argparse
import time

import numpy as np

IDX_BITS = 23
IDX_MASK = (1 << IDX_BITS) - 1
NONE = 0xFFFFFFFF
IDLE = 0x7F7F7F7F
LIMIT = 0x7F000000           # bound[] holds keys below this
NO_X = NONE >> IDX_BITS      # 511: everything passes
# the gate groups of a fired 32x32 tile (bf_mx32.hip: MX32_GATES, mx32_gate_index): accumulator indices
GATE_GROUPS = ((0, 1, 14, 15), (2, 3, 4), (5, 6, 7), (8, 9, 10), (11, 12, 13))
STAGE = 128
EARLY = 0x16                 # SLAM_MX_EARLY: exchanges after 128, 256 and 512 scanned rows
GEOMETRY = {32: (2, 16), 16: (4, 4)}      # tile -> (lanes per query, rows per lane and group)


def plan_table(n, m, num_cu=256, resident=4, workers=None):
    """make_mx_plan_core: (chunk boundaries, workers) for n x m; `workers` overrides the count (one query block of a larger launch)."""
    qblocks = (n + 255) // 256
    w = min(max(num_cu * resident // qblocks, 1), 256) if workers is None else workers
    c = 1024 if m // w >= 8192 else 256
    tbl, at = [0], 0
    while at < m:
        ln = c
        g = (m - at) // (2 * w) // STAGE * STAGE
        if g < ln:
            ln = max(g, STAGE)
        at = min(at + ln, m)
        tbl.append(at)
    return tbl, min(w, len(tbl) - 1)


def bench_rows(n, m, seed_q=228, seed_t=229):
    """The first n query rows and m train rows of the generator bench.py and tools/ab_time.py use."""
    q = np.random.default_rng(seed_q).integers(0, 256, (n, 32), dtype=np.uint8)
    t = np.random.default_rng(seed_t).integers(0, 256, (m, 32), dtype=np.uint8)
    return q, t


def distances(q, t):
    """Hamming distances [n, m] as the kernels get them: (256 - <q+-, t+->) / 2, exact in f32."""
    a = 1.0 - 2.0 * np.unpackbits(q, axis=1).astype(np.float32)
    b = 1.0 - 2.0 * np.unpackbits(t, axis=1).astype(np.float32)
    return ((256 - (a @ b.T)) / 2).astype(np.int64)


def full_sort(d):
    """The two smallest keys (dist << 23 | row) per query: ties go to the lower row."""
    keys = (d << IDX_BITS) | np.arange(d.shape[1], dtype=np.int64)[None, :]
    k = np.sort(keys, axis=1)[:, :2]
    if k.shape[1] < 2:
        k = np.concatenate([k, np.full((len(k), 2 - k.shape[1]), NONE, np.int64)], axis=1)
    return k


def bound_x(g, c0):
    """mx_bound_x: the exclusive threshold a key read from bound[] allows from row c0 on."""
    g = np.asarray(g, np.int64)
    return np.where(g < LIMIT, (g >> IDX_BITS) + np.where((g & IDX_MASK) < c0, 0, 1), NO_X)


class Search:
    """One query block (d: distances [n, m], n a multiple of 64) searched by `workers` workers over the chunks of `tbl`."""

    def __init__(self, d, tbl, workers, tile=32, union=True, carry="none", early=EARLY, log=False):
        assert d.shape[0] % 64 == 0 and tile in GEOMETRY and carry in ("none", "whole", "across_exchange")
        assert carry == "none" or tile == 32, "the carried fold is the 32x32 trip's"
        self.d, self.tbl, self.W, self.tile, self.union, self.carry, self.early = d, list(tbl), workers, tile, union, carry, early
        self.nq, self.m = d.shape
        self.L, self.R = GEOMETRY[tile]
        self.G = self.L * self.R
        self.T = self.nq // tile
        # offs[l, k]: the row of the group that lane l holds at accumulator index k
        k = np.arange(self.R)
        self.offs = np.stack([8 * (k >> 2) + 4 * l + (k & 3) if tile == 32 else 4 * l + k for l in range(self.L)])
        self.odd = (np.arange(self.T) % 2 == 1) if tile == 32 else np.zeros(self.T, bool)     # a wave's tile 1
        shape = (workers, self.nq, self.L)
        self.b1 = np.full(shape, NONE, np.int64)
        self.b2 = self.b1.copy()
        self.x = np.full(shape, NO_X, np.int64)
        self.bound = np.full(self.nq, IDLE, np.int64)
        self.history = [self.bound.copy()]
        self.ticket = 0
        self.nchunks = len(self.tbl) - 1
        self.next = [None] * workers          # the ticket a worker holds for its next chunk
        self.at = [None] * workers            # (chunk, first row of the stage to come) of the chunk it is in
        self.scanned = [0] * workers
        self.pending = [None] * workers       # a carried fold: (s0, group)
        self.done = [False] * workers
        self.folds = self.fired = self.gates = self.unions = self.union_stages = self.block_stages = self.exchanges = 0
        self.tile_stages = self.carried = 0
        self.open_groups = self.group_rows = 0      # tile 32: the gate groups of bf_mx32.hip that the open row gates lie in
        self.fired_log = []                   # (worker, stage start, group, tile) of every fire, in program order per tile
        self.x_log = {} if log else None      # (worker, stage start, group, tile parity) -> the thresholds behind that fold

    # -- pieces ----------------------------------------------------------------------------------------------------------
    def unite(self, w):
        k = np.sort(np.concatenate([self.b1[w], self.b2[w]], axis=1), axis=1)
        return k[:, 0], k[:, 1]

    def draw(self, w):
        self.next[w] = self.ticket
        self.ticket += 1

    def exchange(self, w, c0, deliver):
        _, u2 = self.unite(w)
        g = {"fresh": self.bound, "stale": self.history[max(0, len(self.history) - 4)], "never": self.history[0]}[deliver].copy()
        pub = (u2 < g) & (u2 < LIMIT)
        self.bound = np.where(pub, np.minimum(self.bound, u2), self.bound)
        self.history.append(self.bound.copy())
        self.x[w] = np.minimum(self.x[w], np.minimum(bound_x(g, c0), u2 >> IDX_BITS)[:, None])
        self.exchanges += 1

    def fold(self, w, s0, g, c1, which, stage_fired):
        """Fold group g of the stage at s0 in the tiles `which` [T] of worker w."""
        rows = s0 + g * self.G + self.offs                                   # [L, R]
        valid = rows < c1
        dd = np.where(valid[None], self.d[:, np.minimum(rows, self.m - 1)], 1 << 20)      # [nq, L, R]
        x0 = self.x[w]
        passing = dd < x0[:, :, None]
        if self.tile == 32:
            passing |= (x0 > 129)[:, :, None] & valid[None]
        gate = passing.reshape(self.T, self.tile, self.L, self.R).any(axis=(1, 2))       # [T, R]
        fired = gate.any(axis=1) & which
        self.folds += int(which.sum())
        if fired.any():
            self.fired += int(fired.sum())
            self.gates += int(gate[fired].sum())
            if self.tile == 32:                                              # counted only: the dynamics stay the row gates'
                og = np.stack([gate[:, list(grp)].any(axis=1) for grp in GATE_GROUPS], axis=1)[fired]
                self.open_groups += int(og.sum())
                self.group_rows += int((og * np.array([len(grp) for grp in GATE_GROUPS])).sum())
            self.fired_log += [(w, s0, g, int(t)) for t in np.flatnonzero(fired)]
            stage_fired |= fired
            keys = np.where(valid[None], (dd << IDX_BITS) | rows[None], NONE)
            b1, b2 = self.b1[w], self.b2[w]
            for k in range(self.R):                                          # a lane's rows ascend with the accumulator index
                sel = np.repeat(gate[:, k] & fired, self.tile)
                if not sel.any():
                    continue
                key = keys[sel, :, k]
                lo, hi = np.minimum(b1[sel], b2[sel]), np.maximum(b1[sel], b2[sel])
                b2[sel] = np.maximum(lo, np.minimum(hi, key))                # umed3
                b1[sel] = np.minimum(b1[sel], key)
            sel = np.repeat(fired, self.tile)
            self.x[w][sel] = np.minimum(self.x[w][sel], b2[sel] >> IDX_BITS)
        if self.x_log is not None:
            for par in (0, 1):
                m = which & (self.odd == bool(par))
                if m.any():
                    self.x_log[(w, s0, g, par)] = self.x[w][np.repeat(m, self.tile)].copy()

    # -- a worker's life, one stage per step -------------------------------------------------------------------------------
    def step(self, w, deliver="fresh"):
        """Advance worker w by one stage (with the chunk start in front of a chunk's first).  False once it has run dry."""
        if self.done[w]:
            return False
        if self.at[w] is None:
            if self.next[w] is None:
                self.draw(w)
            ci, self.next[w] = self.next[w], None
            if ci >= self.nchunks:
                self.done[w] = True
                return False
            self.at[w] = (ci, self.tbl[ci])
            self.exchange(w, self.tbl[ci], deliver)
        ci, s0 = self.at[w]
        c1 = self.tbl[ci + 1]
        s1 = s0 + STAGE
        more = s1 < c1
        if not more:
            self.draw(w)                                                     # the next ticket, while the chunk's last stage is scanned
        every = np.ones(self.T, bool)
        stage_fired = np.zeros(self.T, bool)
        groups = (min(s1, c1) - s0 + self.G - 1) // self.G
        after = self.scanned[w] + min(s1, c1) - s0
        early = more and after < 32 * STAGE and bool(self.early >> (after // STAGE) & 1)
        carry = self.carry != "none" and more and (self.carry == "across_exchange" or not early)
        for g in range(groups):
            if g == 0 and self.pending[w] is not None:                       # behind t0k0 .. t0k3 of group 0: tile 0 is not folded yet
                ps0, pg = self.pending[w]
                self.fold(w, ps0, pg, c1, self.odd, np.zeros(self.T, bool))
                self.pending[w] = None
            last = carry and g == groups - 1
            self.fold(w, s0, g, c1, ~self.odd if last else every, stage_fired)
            if last:
                self.pending[w] = (s0, g)
                self.carried += 1
        self.block_stages += 1
        self.tile_stages += self.T
        if self.union and stage_fired.any():
            _, u2 = self.unite(w)
            sel = np.repeat(stage_fired, self.tile)
            self.x[w][sel] = np.minimum(self.x[w][sel], (u2[sel] >> IDX_BITS)[:, None])
            self.unions += int(stage_fired.sum())
            self.union_stages += 1
        self.scanned[w] = after
        if early:
            self.exchange(w, s1, deliver)
        self.at[w] = (ci, s1) if more else None
        return True

    def equal_rate(self, deliver="fresh"):
        for w in range(self.W):
            self.draw(w)
        live = True
        while live:
            live = False
            for w in range(self.W):
                live |= self.step(w, deliver)
        return self

    def result(self):
        assert all(p is None for p in self.pending), "a carried fold was never run"
        k = np.concatenate([self.b1.transpose(1, 0, 2).reshape(self.nq, -1), self.b2.transpose(1, 0, 2).reshape(self.nq, -1)], axis=1)
        return np.sort(k, axis=1)[:, :2]

    def counts(self):
        return {"tile_groups": self.folds, "fired": self.fired, "open_gates_per_fired_tile": self.gates / max(self.fired, 1),
                "unions": self.unions, "tile_stages": self.tile_stages, "block_stages_with_a_union": self.union_stages,
                "block_stages": self.block_stages, "exchanges": self.exchanges,
                "open_groups_per_fired_tile": self.open_groups / max(self.fired, 1),
                "rows_of_open_groups_per_fired_tile": self.group_rows / max(self.fired, 1)}


def run(d, tile, union, workers=None, plan_n=None, cus=256, carry="none"):
    n, m = d.shape
    tbl, w = plan_table(plan_n or n, m, cus, 4, workers)
    s = Search(d, tbl, w, tile, union, carry).equal_rate()
    assert np.array_equal(s.result(), full_sort(d)), "the model's table is not the full sort"
    return s


def line(label, s):
    c = s.counts()
    return (f"{label:<44} fired {c['fired']:5d} of {c['tile_groups']:6d} tile-groups ({100 * c['fired'] / c['tile_groups']:4.1f} %), "
            f"{c['open_gates_per_fired_tile']:5.2f} of {s.R} gates open per fired tile, unions {c['unions']:5d} of {c['tile_stages']:5d} tile-stages "
            f"({c['block_stages_with_a_union']} of {c['block_stages']} block-stages), exchanges {c['exchanges']}"
            + (f", {c['open_groups_per_fired_tile']:4.2f} of {len(GATE_GROUPS)} gate groups open holding "
               f"{c['rows_of_open_groups_per_fired_tile']:4.2f} rows" if s.tile == 32 else ""))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--tile", type=int, choices=(16, 32))
    ap.add_argument("--union", choices=("on", "off"), default="on")
    ap.add_argument("--workers", type=int)
    ap.add_argument("--plan-n", type=int)
    ap.add_argument("--cus", type=int, default=256)
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--m", type=int, default=65536)
    ap.add_argument("--seed-q", type=int, default=228)
    ap.add_argument("--seed-t", type=int, default=229)
    a = ap.parse_args()
    t0 = time.time()
    d = distances(*bench_rows(a.n, a.m, a.seed_q, a.seed_t))
    if a.tile:
        s = run(d, a.tile, a.union == "on", a.workers, a.plan_n, a.cus)
        print(line(f"{a.tile}x{a.tile}, {s.W} workers, union {a.union}", s))
    else:
        for tile, w in ((32, 4), (16, 4), (16, 1)):
            for union in (True, False):
                s = run(d, tile, union, w)
                print(line(f"{tile}x{tile}, {w} worker{'s' if w > 1 else ''}, {'unions per stage' if union else 'no per-stage union'}", s), flush=True)
    print(f"every table equalled the full sort ({a.n} queries x {a.m} rows, seeds {a.seed_q} / {a.seed_t}; {time.time() - t0:.0f} s)")


if __name__ == "__main__":
    main()
