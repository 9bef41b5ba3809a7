"""CPU suite: the stage tail of the matrix-core top-2 searches (bf_mx32.hip, bf_mx.hip) without a GPU.

1. tools/mx_fire_model.py - the numpy restatement of both kernels' threshold schedule - gives the full sort (ties to the lower
   row) WITHOUT the per-stage union of a query's lanes, in both geometries, on the tie-heavy families of tests/test_mx_ties_cpu.py
   (few-valued, duplicated, all-equal rows) and on random rows, for one worker and many, workers in turn and a racing one, fresh,
   stale and never-delivered bounds.
2. The carried fold (tile 1 of a stage's last group folded behind the next stage's first four MFMAs: described in DESIGN.md 3c,
   NOT in the kernel - tests/test_mx32_pipe_cpu.py holds every trip to one bare fold) replayed from the model's explicit order:
   same tables, same thresholds behind every fold, same fired list as the bare order where no early exchange stands at the stage
   end; carried ACROSS an early exchange it loses a tie it must win, and the case that shows it is constructed here.
3. The model's counts on the benchmark's rows are pinned (the schedule is deterministic): the figures of DESIGN.md.
4. The built 32x32 kernel: the limits the existing ISA tests state, exactly one bare fold per trip, and no `ds_bpermute_b32`
   between a trip's last MFMA and the stage barrier except the early exchange's own."""
import importlib.util
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from test_mx32_cpu import field, mx32_kernel  # noqa: F401  (the kernel's disassembly and metadata, as that suite obtains them)
from test_mx32_pipe_cpu import _folds, _regs, _trips

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("mx_fire_model", os.path.join(ROOT, "tools", "mx_fire_model.py"))
fm = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(fm)

OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
NQ = 64


# ---- data: the families of tests/test_mx_ties_cpu.py ---------------------------------------------------------------------

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
SIZES = [(1, 640), (3, 1024), (4, 1000), (7, 1413), (1, 8192 + 300)]     # (workers, train rows): the last has eight-stage chunks


# ---- schedules -----------------------------------------------------------------------------------------------------------

def in_turn(s, deliver="fresh"):
    s.equal_rate(deliver)


def racing(s, deliver="fresh", lead=6):
    """Every worker but the last holds the ticket it drew and stalls in front of its chunk start; the last one runs `lead`
    stages - whole chunks among them, and publishes from them - before the stalled ones read bound[] for their LOWER chunks and
    scan them.  Repeated until the queue is dry."""
    for w in range(s.W):
        s.draw(w)
    live = True
    while live:
        live = False
        for _ in range(lead):
            live |= s.step(s.W - 1, deliver)
        for w in range(s.W - 1):
            while s.step(w, deliver):
                live = True
                if s.at[w] is None:                # its chunk is done; it holds the next ticket
                    break


def cases(tile, union, families=FAMILIES, schedules=(in_turn, racing), delivers=("fresh", "stale", "never"), carry="none", log=False):
    for fam in families:
        for si, (workers, m) in enumerate(SIZES):
            if carry != "none" and workers > 1:
                continue
            rng = np.random.default_rng(100 * FAMILIES.index(fam) + si)
            d = fm.distances(*fam(rng, NQ, m))
            tbl, w = fm.plan_table(NQ, m, workers=workers)
            for sched in schedules:
                for deliver in delivers:
                    s = fm.Search(d, tbl, w, tile, union, carry, log=log)
                    sched(s, deliver)
                    yield f"{fam.__name__}/{sched.__name__}/{deliver}/{workers}x{m}", s, fm.full_sort(d)


# ---- 1. no per-stage union -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tile", [32, 16])
@pytest.mark.parametrize("fam", FAMILIES, ids=lambda f: f.__name__)
def test_without_the_per_stage_union_the_tables_are_the_full_sort(tile, fam):
    n = 0
    for name, s, ref in cases(tile, False, families=[fam]):
        assert np.array_equal(s.result(), ref), name
        assert s.unions == 0 and s.exchanges > 0
        n += 1
    assert n == len(SIZES) * 6


@pytest.mark.parametrize("tile", [32, 16])
def test_with_the_union_the_model_is_the_same_search_and_fires_no_more(tile):
    """The comparison the change rests on is between two right answers: the union only ever lowers a threshold."""
    for fam in (random_rows, duplicates):
        with_u = {name: s for name, s, _ in cases(tile, True, families=[fam], schedules=(in_turn,), delivers=("fresh",))}
        for name, s, ref in cases(tile, False, families=[fam], schedules=(in_turn,), delivers=("fresh",)):
            assert np.array_equal(with_u[name].result(), ref), name
            assert with_u[name].fired <= s.fired, name
            assert (with_u[name].x <= s.x).all(), name


def test_the_plan_restated_is_the_library_s(built):
    import slamhip

    for n, m in ((65536, 65536), (8192, 65536), (300, 16461), (64, 16461), (513 * 256, 10057), (1 << 20, 1 << 20), (500, 200000)):
        plan, tbl = slamhip.mx_plan_describe(n, m, num_cu=256)
        got, w = fm.plan_table(n, m, 256, plan["resident"])
        assert got == list(tbl) and w == plan["workers"], (n, m)


# ---- 2. the carried fold ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fam", FAMILIES, ids=lambda f: f.__name__)
def test_a_fold_carried_where_no_exchange_follows_changes_only_when_it_runs(fam):
    bare = {name: s for name, s, _ in cases(32, False, families=[fam], schedules=(in_turn,), carry="none", log=True)}
    carried_stages = 0
    for name, s, ref in cases(32, False, families=[fam], schedules=(in_turn,), carry="whole", log=True):
        b = bare[name]
        assert np.array_equal(s.result(), ref), name
        assert np.array_equal(s.b1, b.b1) and np.array_equal(s.b2, b.b2) and np.array_equal(s.x, b.x), name
        for tile in range(s.T):                       # a tile's fires, in the tile's own order
            assert [e for e in s.fired_log if e[3] == tile] == [e for e in b.fired_log if e[3] == tile], (name, tile)
        assert sorted(s.fired_log) == sorted(b.fired_log)
        assert s.x_log.keys() == b.x_log.keys()
        for key in s.x_log:                           # (worker, stage, group, tile parity): the thresholds behind that fold
            assert np.array_equal(s.x_log[key], b.x_log[key]), (name, key)
        assert b.carried == 0
        carried_stages += s.carried                   # the one difference: when those folds ran
    assert carried_stages > 50


def _tie_across_an_early_exchange():
    """Query 40 (tile 1 of its wave) is w, every other query v.  Rows 0, 1, 4 and 6 bring both lanes of every v query down to
    distance 1 in the first group, so the random rows behind never open a gate for them.  For w, row 5 is w itself and rows 100
    and 120 - both in the last group of stage 0 - are at distance 6; everything else is far.  The right table of query 40 is
    rows 5 and 100.  bound[40] holds the key of row 120, distance 6, a valid bound (the final 2nd-best key is (6, 100), below
    it): the key of a higher row, below the next stage's first row 128.  In the kernel no other worker scans that group, so no
    launch delivers this key; the restriction the header states is against exactly this reading of the bound, and the model is
    handed it directly."""
    rng = np.random.default_rng(40)
    q, t = random_rows(rng, NQ, 640)

    def at(row, dist):
        bits = np.unpackbits(row)
        bits[rng.permutation(256)[:dist]] ^= 1
        return np.packbits(bits)

    v, w = q[0].copy(), q[40].copy()
    q[:] = v
    q[40] = w
    t[0], t[1], t[4], t[6] = v, at(v, 1), v, at(v, 1)
    t[5], t[100], t[120] = w, at(w, 6), at(w, 6)
    d = fm.distances(q, t)
    tbl, w = fm.plan_table(NQ, 640, workers=1)
    assert tbl[1] == 256, "stage 0 is followed by a stage of its chunk, with the early exchange after 128 rows between them"
    return d, tbl, w


@pytest.mark.parametrize("carry,right", [("none", True), ("whole", True), ("across_exchange", False)])
def test_a_fold_carried_across_an_early_exchange_loses_a_tie_it_must_win(carry, right):
    d, tbl, w = _tie_across_an_early_exchange()
    s = fm.Search(d, tbl, w, 32, False, carry)
    s.bound[40] = (6 << fm.IDX_BITS) | 120
    s.history = [s.bound.copy()]
    s.equal_rate()
    ref = fm.full_sort(d)
    assert ref[40].tolist() == [5, (6 << fm.IDX_BITS) | 100]
    got = s.result()
    assert np.array_equal(got, ref) == right, (carry, got[40], ref[40])
    if not right:
        assert got[40, 0] == 5 and got[40, 1] != ref[40, 1]          # the tie at the lower row was dropped
        assert np.array_equal(np.delete(got, 40, axis=0), np.delete(ref, 40, axis=0))


# ---- 3. the counts on the benchmark's rows -----------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def bench_distances():
    return fm.distances(*fm.bench_rows(256, 65536))


@pytest.mark.parametrize("tile,union,fired,unions,union_stages", [
    (32, True, 2901, 1666, 467),
    (32, False, 2962, 0, 0),
    (16, True, 4345, 2238, 467),
    (16, False, 4563, 0, 0),
])
def test_counts_on_the_benchmark_rows(bench_distances, tile, union, fired, unions, union_stages):
    """One query block of the headline launch: 256 queries (seed 228) x 65536 rows (seed 229), 4 workers, 1024-row chunks."""
    s = fm.run(bench_distances, tile, union, workers=4)
    c = s.counts()
    print(fm.line(f"{tile}x{tile}, union {union}", s))
    assert c["tile_groups"] == (16384 if tile == 32 else 65536) and c["block_stages"] == 512
    assert (c["fired"], c["unions"], c["block_stages_with_a_union"]) == (fired, unions, union_stages)


# ---- 4. the built kernel -----------------------------------------------------------------------------------------------------

def program(lib_path, tmp):
    """[(address, instruction)] of bf_top2_mx32_kernel in the library at lib_path, in program order."""
    local = os.path.join(tmp, "lib.so")
    shutil.copy(lib_path, local)
    subprocess.run([OBJDUMP, "--offloading", local], cwd=tmp, check=True, capture_output=True)
    for f in sorted(os.listdir(tmp)):
        if "gfx950" not in f:
            continue
        text = subprocess.run([OBJDUMP, "-d", os.path.join(tmp, f)], check=True, capture_output=True, text=True).stdout
        m = re.search(r"^[0-9a-f]+ <(_Z\d+bf_top2_mx32_kernel\w*)>:$", text, re.M)
        if not m:
            continue
        out = []
        for ln in text[m.end():].split("\n\n", 1)[0].splitlines():
            code, _, note = ln.partition("//")
            if code.strip():
                out.append((int(note.split(":")[0], 16), code.strip()))
        return out
    pytest.fail("bf_top2_mx32_kernel is not in the library")


def bpermutes_to_the_barrier(prog, start):
    """The numbers of `ds_bpermute_b32` a wave can execute from instruction index `start` to the first `s_barrier` it reaches:
    every path through the branches, as a set (counts above 32 are not told apart)."""
    at = {a: i for i, (a, _) in enumerate(prog)}
    seen, work, out = {}, [(start, 0)], set()
    while work:
        i, n = work.pop()
        if n in seen.setdefault(i, set()) or n > 32:
            continue
        seen[i].add(n)
        addr, ins = prog[i]
        op = ins.split()[0]
        if op == "s_barrier":
            out.add(n)
            continue
        if op == "s_endpgm":
            continue
        n += op == "ds_bpermute_b32"
        nxt = []
        if op == "s_branch" or op.startswith("s_cbranch"):
            off = int(ins.split()[1])
            nxt.append(at[addr + 4 + 4 * (off - 65536 if off >= 32768 else off)])
        if op != "s_branch":
            nxt.append(i + 1)
        work += [(j, n) for j in nxt]
    return out


@pytest.fixture(scope="module")
def mx32_program(built, tmp_path_factory):
    if not os.path.exists(OBJDUMP):
        pytest.skip("llvm-objdump of the ROCm toolchain not found")
    from slamhip import _lib

    return program(_lib.LIB_PATH, str(tmp_path_factory.mktemp("mx_stage_tail_isa")))


def test_the_kernel_keeps_the_limits_of_the_existing_isa_tests(mx32_kernel, mx32_program):  # noqa: F811
    body, meta = mx32_kernel
    assert field(meta, "vgpr_count") + field(meta, "agpr_count") <= 128
    assert "scratch_" not in body and "v_accvgpr_" not in body
    for key in ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size"):
        assert field(meta, key) == 0, key
    assert field(meta, "group_segment_fixed_size") <= 40960
    ins = [s for _, s in mx32_program]
    trips = _trips(ins)
    assert len(trips) >= 2
    for trip in trips:
        folds = _folds(ins, trip)
        assert len(folds) == 8
        bare = [f for f in folds if f[2] == trip[-1]]
        assert len(bare) == 1, "no fold is carried: every trip ends with the bare fold of tile 1"
        for i, mine, last in folds:
            assert not re.match(r"s_nop ([4-9]|\d\d)", ins[i - 1]), (ins[i - 1], ins[i])
            if last != trip[-1]:
                between = [j for j in trip if last < j < i]
                assert between and all(set(mine) != _regs(ins[j].split()[1].rstrip(",")) for j in between), ins[i]


def test_no_lane_exchange_between_a_trip_and_the_stage_barrier_but_the_early_exchange(mx32_program):
    """With the per-stage union a wave ran two `ds_bpermute_b32` per fired tile between its last MFMA and `s_barrier` (2 or 4,
    and 6 more where an early exchange followed).  Now every way from a trip's last MFMA to the barrier has none, or the early
    exchange's own six (two unions of two, and the bound's key for either tile)."""
    ins = [s for _, s in mx32_program]
    for trip in _trips(ins):
        counts = bpermutes_to_the_barrier(mx32_program, trip[-1] + 1)
        print("ds_bpermute_b32 from the trip's last MFMA to the barrier, by path:", sorted(counts))
        assert 0 in counts and counts <= {0, 6}, counts
