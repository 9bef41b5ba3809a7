"""CPU suite: the pipelined whole-stage trip of the 32x32x64 matrix-core top-2 search (bf_mx32.hip) without a GPU.

1. A numpy replay of what a wave does to its state - two query tiles, each with its own accumulator register set, per-lane
   top-2 keys and exclusive threshold; rows taken in ascending order through the row gates; the `umed3` / `min` update; the
   union of a query's two lanes after a stage that fired - run from an explicit instruction schedule (MFMAs and folds) under the
   order the kernel had (both folds bunched behind a group's eight MFMAs) and under the pipelined order (whole tile runs, each
   fold behind the four MFMAs of the other tile; and the MFMA-by-MFMA alternation that was measured first), on the tie-heavy
   families of tests/hamming_families.  Tables, thresholds and fired groups must be equal:
   the interleaving between the tiles is immaterial, a tile only ever sees its own operations in their own order.
2. The built kernel's listing, obtained as tests/test_mx32_cpu.py obtains it: in the whole-stage trip at least one MFMA of the
   other tile stands between the last MFMA that writes a tile's accumulators and the first maximum that reads them, and no
   fold is preceded by an `s_nop` of 4 or more.

The lane-half exchange without LDS (`v_permlane32_swap`) was measured and not kept, so nothing is asked about
`ds_bpermute` here."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import hamming_families as hf

LLVM = "/opt/rocm/lib/llvm/bin"
OBJDUMP = os.path.join(LLVM, "llvm-objdump")

STAGE, GROUP, IDX_BITS = 128, 32, 23
KEY_NONE = np.uint32(0xFFFFFFFF)


# ---- the replay ---------------------------------------------------------------------------------------------------------

def bunched(groups):
    """The order before this change: a group's eight MFMAs, K-quarter by K-quarter over both tiles, then both folds."""
    ev = []
    for g in range(groups):
        ev += [("dot", tt, g, kq) for kq in range(4) for tt in range(2)]
        ev += [("fold", 0, g), ("fold", 1, g)]
    return ev


def pipelined(groups):
    """t0k0 t0k1 t0k2 t0k3 [fold t1 of g - 1] t1k0 t1k1 t1k2 t1k3 [fold t0 of g]; tile 1 of the last group folds bare."""
    ev = []
    for g in range(groups):
        ev += [("dot", 0, g, kq) for kq in range(4)]
        if g:
            ev.append(("fold", 1, g - 1))
        ev += [("dot", 1, g, kq) for kq in range(4)]
        ev.append(("fold", 0, g))
    ev.append(("fold", 1, groups - 1))
    return ev


def alternating(groups):
    """The order first measured: t0k0 t0k1 [fold t1 of g - 1] t1k0 t1k1 t0k2 t1k2 t0k3 t1k3 [fold t0 of g]."""
    ev = []
    for g in range(groups):
        ev += [("dot", 0, g, 0), ("dot", 0, g, 1)]
        if g:
            ev.append(("fold", 1, g - 1))
        ev += [("dot", 1, g, 0), ("dot", 1, g, 1), ("dot", 0, g, 2), ("dot", 1, g, 2), ("dot", 0, g, 3), ("dot", 1, g, 3)]
        ev.append(("fold", 0, g))
    ev.append(("fold", 1, groups - 1))
    return ev


def pm1(values):
    """prefix rows as +-1 vectors [n, 256]: a set bit is -1."""
    return 1 - 2 * np.unpackbits(hf.prefix_rows(values), axis=1).astype(np.int64)


def replay(a, b, schedule):
    """One wave (64 queries b) of one worker over the train rows a, stage by stage, each stage run from schedule(groups).
    Returns (b1, b2 [2 tiles, 2 lane halves, 32], x [2, 2, 32], the fired (stage, group, tile) list, the united pairs)."""
    m = len(a)
    tv = np.vstack([pm1(a), np.ones(((-m) % GROUP, 256), np.int64)])      # rows past the end: never enter (index test)
    qv = pm1(b).reshape(2, 32, 256)                                       # tile, column
    b1 = np.full((2, 2, 32), KEY_NONE, np.uint32)
    b2 = b1.copy()
    xs = np.full((2, 2, 32), 511, np.int64)
    fired_log, xs_log = [], []
    for s0 in range(0, m, STAGE):
        groups = (min(m, s0 + STAGE) - s0 + GROUP - 1) // GROUP
        acc = [None, None]                                                # the tile's accumulator registers: [32 rows, 32 columns]
        owner = [None, None]                                              # (group, K-quarters summed) they hold
        fired = set()
        for ev in schedule(groups):
            if ev[0] == "dot":
                _, tt, g, kq = ev
                rows = tv[s0 + g * GROUP:s0 + (g + 1) * GROUP, 64 * kq:64 * kq + 64]
                part = rows @ qv[tt][:, 64 * kq:64 * kq + 64].T
                if kq == 0:
                    acc[tt], owner[tt] = part, (g, 1)                     # C = inline 0: whatever was there is gone
                else:
                    assert owner[tt] == (g, kq), "a K-quarter accumulates onto its own group's earlier quarters"
                    acc[tt], owner[tt] = acc[tt] + part, (g, kq + 1)
                continue
            _, tt, g = ev
            assert owner[tt] == (g, 4), "a fold reads the four quarters of the group it folds"
            dist = (256 - acc[tt]) // 2                                   # [row of the group, column]
            x0 = xs[tt].copy()
            took = False
            # lane (hk, col) holds rows 8 i + 4 hk + j, ascending with the accumulator index 4 i + j
            offs = [[8 * (k >> 2) + 4 * hk + (k & 3) for k in range(16)] for hk in range(2)]
            for k in range(16):
                d = np.stack([dist[offs[hk][k]] for hk in range(2)])      # [lane half, column]
                if not ((d < x0) | (x0 > 129)).any():                     # the row gate: all lanes of the tile or none; above
                    # 129 the kernel's pattern is INT_MIN and everything passes (the update is exact whatever passes)
                    continue
                took = True
                for hk in range(2):
                    row = s0 + g * GROUP + offs[hk][k]
                    key = ((d[hk] << IDX_BITS) | row).astype(np.uint32) if row < m else np.full(32, KEY_NONE, np.uint32)
                    lo, hi = np.minimum(b1[tt, hk], b2[tt, hk]), np.maximum(b1[tt, hk], b2[tt, hk])
                    b2[tt, hk] = np.maximum(lo, np.minimum(hi, key))      # umed3
                    b1[tt, hk] = np.minimum(b1[tt, hk], key)
            if took:
                fired.add(tt)
                fired_log.append((s0 // STAGE, g, tt))
                xs[tt] = np.minimum(xs[tt], (b2[tt] >> IDX_BITS).astype(np.int64))
        for tt in sorted(fired):                                          # the stage end sees both tiles fully folded
            u2 = np.minimum(np.maximum(b1[tt, 0], b1[tt, 1]), np.minimum(b2[tt, 0], b2[tt, 1]))
            xs[tt] = np.minimum(xs[tt], (u2 >> IDX_BITS).astype(np.int64)[None, :])
        xs_log.append(xs.copy())
    u1 = np.minimum(b1[:, 0], b1[:, 1])
    u2 = np.minimum(np.maximum(b1[:, 0], b1[:, 1]), np.minimum(b2[:, 0], b2[:, 1]))
    return b1, b2, np.array(xs_log), fired_log, (u1.reshape(64), u2.reshape(64))


M = 3 * STAGE + 77                                                        # three whole stages and a short one with a ragged tail
RNG = np.random.default_rng(3264)
FAMILIES = {
    "constant0": (hf.constant(M, 0), hf.queries_equal(64)),
    "constant256_vs_0": (hf.constant(M, 256), hf.queries_equal(64)),
    "ladder_asc": (hf.ladder(M, "asc"), hf.queries_ramp(64)),
    "ladder_desc_alternating": (hf.ladder(M, "desc"), hf.queries_alternating(64)),
    "ladder_perm": (hf.ladder(M, "perm"), hf.queries_ramp(64) * 4),
    "alphabet2": (hf.alphabet(M, (7, 250), RNG), hf.queries_ramp(64)),
    "alphabet3": (hf.alphabet(M, (0, 128, 256), RNG), hf.queries_alternating(64)),
    "plateau_across_a_stage": (hf.plateau_case(M, 2, 5, STAGE)[0], hf.queries_equal(64)),
    "plateau_across_a_group": (hf.plateau_case(M, 2, 128, STAGE + 3 * GROUP)[0], hf.queries_equal(64)),
}


def test_each_tile_sees_its_own_operations_in_the_same_order():
    for groups in (1, 2, 3, 4):
        for tt in range(2):
            old = [e for e in bunched(groups) if e[1] == tt]
            for order in (pipelined, alternating):
                new = [e for e in order(groups) if e[1] == tt]
                assert old == new and len(new) == 5 * groups


def test_a_pipelined_fold_stands_behind_an_mfma_of_the_other_tile():
    ev = pipelined(4)
    for i, e in enumerate(ev):
        if e[0] != "fold":
            continue
        last = max(j for j in range(i) if ev[j][0] == "dot" and ev[j][1] == e[1])
        assert any(x[0] == "dot" and x[1] != e[1] for x in ev[last + 1:i]) or e == ("fold", 1, 3), e


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_interleaving_between_the_tiles_is_immaterial(family):
    a, b = FAMILIES[family]
    old, new = replay(a, b, bunched), replay(a, b, pipelined)
    alt = replay(a, b, alternating)
    assert all(np.array_equal(x, y) for x, y in zip(alt[:3], new[:3])) and alt[3] == new[3]
    assert np.array_equal(old[0], new[0]) and np.array_equal(old[1], new[1]), "tables"
    assert np.array_equal(old[2], new[2]), "thresholds after every stage"
    assert old[3] == new[3] and len(new[3]) > 0, "fired (stage, group, tile)"
    # and the replay is the search: the united pairs are the integer expectation, ties to the lower row
    idx, dist = hf.expected_topk(a, b, 2)
    for u, col in ((new[4][0], 0), (new[4][1], 1)):
        assert np.array_equal((u & np.uint32((1 << IDX_BITS) - 1)).astype(np.int32), idx[:, col])
        assert np.array_equal((u >> IDX_BITS).astype(np.int32), dist[:, col])


# ---- the built kernel ---------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def listing(built, tmp_path_factory):
    """The instructions of bf_top2_mx32_kernel in the library the package loads, in program order."""
    if not os.path.exists(OBJDUMP):
        pytest.skip("llvm-objdump of the ROCm toolchain not found")
    from slamhip import _lib

    tmp = str(tmp_path_factory.mktemp("mx32_pipe_isa"))
    local = os.path.join(tmp, "lib.so")
    shutil.copy(_lib.LIB_PATH, local)
    subprocess.run([OBJDUMP, "--offloading", local], cwd=tmp, check=True, capture_output=True)
    for f in sorted(os.listdir(tmp)):
        if "gfx950" not in f:
            continue
        text = subprocess.run([OBJDUMP, "-d", os.path.join(tmp, f)], check=True, capture_output=True, text=True).stdout
        m = re.search(r"^[0-9a-f]+ <(_Z\d+bf_top2_mx32_kernel\w*)>:$", text, re.M)
        if m:
            body = text[m.end():].split("\n\n", 1)[0]
            return [ln.split("//")[0].strip() for ln in body.splitlines() if ln.split("//")[0].strip()]
    pytest.fail("bf_top2_mx32_kernel is not in the library")


def _regs(tok):
    m = re.match(r"v\[(\d+):(\d+)\]", tok)
    if m:
        return set(range(int(m.group(1)), int(m.group(2)) + 1))
    m = re.match(r"v(\d+)$", tok)
    return {int(m.group(1))} if m else set()


def _trips(ins):
    """The whole-stage trips: runs of 32 MFMAs (four groups of eight, eight of them from C = 0) with fewer than 40
    instructions between neighbours - the update paths lie out of line - as lists of instruction indices.  The short last
    stage is a loop of one group, eight MFMAs, and is no trip."""
    at = [i for i, s in enumerate(ins) if s.startswith("v_mfma")]
    runs, cur = [], [at[0]]
    for i in at[1:]:
        if i - cur[-1] < 40:
            cur.append(i)
        else:
            runs.append(cur)
            cur = [i]
    runs.append(cur)
    first = lambda i: bool(re.search(r"\], 0 cbsz:4", ins[i]))       # a tile's first K-quarter starts from inline 0
    trips = [r[k:k + 32] for r in runs if len(r) % 32 == 0 for k in range(0, len(r), 32)]   # two trips may lie back to back
    return [r for r in trips if first(r[0]) and sum(first(i) for i in r) == 8]


def _folds(ins, trip):
    """(index of the first maximum, the accumulator set it reads, index of the last MFMA that writes it) of the trip's folds."""
    sets = sorted({tuple(sorted(_regs(ins[i].split()[1].rstrip(",")))) for i in trip})
    assert len(sets) == 2, "two accumulator sets, one per tile"
    out = []
    end = min(trip[-1] + 40, len(ins))
    for i in range(trip[0], end):
        if not ins[i].startswith("v_max_i32"):
            continue
        src = set().union(*(_regs(t.rstrip(",")) for t in ins[i].split()[2:]))
        mine = [s for s in sets if src and src <= set(s)]
        if not mine:
            continue
        writers = [j for j in trip if j < i and set(mine[0]) == _regs(ins[j].split()[1].rstrip(","))]
        out.append((i, mine[0], writers[-1]))
    return out


def test_the_trips_are_found(listing):
    trips = _trips(listing)
    assert len(trips) >= 2, "a trip that stages the next stage and one that does not"
    for trip in trips:
        assert len(_folds(listing, trip)) == 8, "two folds per group"


def test_every_fold_of_a_trip_stands_behind_an_mfma_of_the_other_tile(listing):
    for trip in _trips(listing):
        bare = 0
        for i, mine, last in _folds(listing, trip):
            if last == trip[-1]:                                 # tile 1 of the last group: nothing of the stage is left to issue
                bare += 1
                continue
            between = [j for j in trip if last < j < i]
            assert between and all(set(mine) != _regs(listing[j].split()[1].rstrip(",")) for j in between), listing[i]
        assert bare == 1


def test_no_fold_of_a_trip_is_preceded_by_a_long_nop(listing):
    """gfx950 does not interlock a vector read of an MFMA result: the compiler owes 11 wait states between the last 8-pass MFMA
    that writes the accumulators and the first maximum, counts every instruction between them as ONE state, and pads the rest
    with `s_nop`.  With the tiles alternating MFMA by MFMA one MFMA stood between them and every fold of tile 0 followed
    `s_nop 9`; with whole tile runs four MFMAs and the other fold do (the first group's fold of tile 0, behind four MFMAs and
    four operand reads, keeps `s_nop 3`)."""
    bad = []
    for trip in _trips(listing):
        for i, _, _ in _folds(listing, trip):
            m = re.match(r"s_nop (\d+)", listing[i - 1])
            if m and int(m.group(1)) >= 4:
                bad.append((listing[i - 1], listing[i]))
    print(len(bad), "folds behind a long s_nop:", bad)
    assert not bad
