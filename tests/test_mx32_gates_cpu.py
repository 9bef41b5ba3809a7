"""CPU suite: the group gates of a fired tile of the 32x32x64 matrix-core top-2 search (bf_mx32_scan.inc) without a GPU.

1. The partition of the accumulator indices 0 .. 15 into gate groups, and its map to the rows of a group.
2. A numpy replay of a wave's two tiles (the state model of tests/test_mx32_pipe_cpu.py: per lane a sorted pair of keys and an
   exclusive threshold distance, a lane half holding rows 8 (i >> 2) + 4 hk + (i & 3)) in which a fired tile lets rows in
     "rows": through the 16 row gates the kernel had - a row enters where some lane of the tile passes at it;
     "a":    through the group gates, then the row gates inside an open group;
     "b":    through the group gates alone - every row of an open group enters (what the kernel does);
   on the tie families and on random rows, one worker and several.  "a" must be "rows" move for move; "b" must give the full
   sort's tables with thresholds never looser than "a"'s and publish only keys of real rows.  A partition that leaves an index
   out is caught by the same checks.
3. The built listing of both kernels: the limits of the existing listing tests, the gate compares ahead of a fired block's first
   scalar test, and the eight maxima of a quiet fold."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import hamming_families as hf
import test_mx32_pipe_cpu as pipe

LLVM = "/opt/rocm/lib/llvm/bin"
OBJDUMP, READELF = os.path.join(LLVM, "llvm-objdump"), os.path.join(LLVM, "llvm-readelf")

STAGE, GROUP, IDX_BITS = 128, 32, 23
KEY_NONE = np.uint32(0xFFFFFFFF)
# bf_mx32.hip: MX32_GATES, mx32_gate_rows, mx32_gate_index
GATE_GROUPS = ((0, 1, 14, 15), (2, 3, 4), (5, 6, 7), (8, 9, 10), (11, 12, 13))
ROW_GATES = tuple((i,) for i in range(16))


def row_of(i, hk):
    return 8 * (i >> 2) + 4 * hk + (i & 3)


# ---- the partition --------------------------------------------------------------------------------------------------------

def test_the_partition_covers_every_accumulator_index_once():
    flat = [i for g in GATE_GROUPS for i in g]
    assert sorted(flat) == list(range(16)) and 4 <= len(GATE_GROUPS) <= 6
    # as the kernel's text computes it
    rows = lambda j: 3 if j else 4
    index = lambda j, r: 3 * j - 1 + r if j else (r if r < 2 else 12 + r)
    assert tuple(tuple(index(j, r) for r in range(rows(j))) for j in range(5)) == GATE_GROUPS
    src = open(os.path.join(os.path.dirname(__file__), "..", "slam-experiments_amd", "csrc", "bf_mx32.hip")).read()
    assert "#define MX32_GATES 5" in src
    assert "mx32_gate_rows(int j) { return j ? 3 : 4; }" in src
    assert "mx32_gate_index(int j, int r) { return j ? 3 * j - 1 + r : (r < 2 ? r : 12 + r); }" in src


def test_an_index_maps_to_its_row_of_the_group():
    for hk in range(2):
        rows = [row_of(i, hk) for i in range(16)]
        assert rows == sorted(rows), "a lane's rows ascend with the accumulator index"
    assert sorted(row_of(i, hk) for i in range(16) for hk in range(2)) == list(range(GROUP))
    assert [row_of(i, 1) for i in (0, 3, 4, 15)] == [4, 7, 12, 31]


# ---- the replay -----------------------------------------------------------------------------------------------------------

def replay(dist, mode, groups=GATE_GROUPS, lo=0, hi=None):
    """One worker's wave over the train rows lo .. hi of dist [m, 64 queries].  Returns (b1, b2 [2 tiles, 2 halves, 32], the
    thresholds after every (stage, group, tile), the fired list, the entering indices per fire)."""
    m = len(dist)
    hi = m if hi is None else hi
    assert lo % STAGE == 0
    if mode == "rows":
        groups = ROW_GATES
    b1 = np.full((2, 2, 32), KEY_NONE, np.uint32)
    b2 = b1.copy()
    xs = np.full((2, 2, 32), 511, np.int64)
    xs_log, fired, entered = [], [], []
    for g0 in range(lo, hi, GROUP):
        for tt in range(2):
            x0 = xs[tt].copy()                                             # every gate sees the threshold as it stood at the fold
            d = np.full((16, 2, 32), 1 << 20, np.int64)                    # [index, lane half, column]
            for i in range(16):
                for hk in range(2):
                    r = g0 + row_of(i, hk)
                    # rows past the train set are zero rows to the MFMA: any distance; what matters is that their key is NONE
                    d[i, hk] = dist[r, 32 * tt:32 * tt + 32] if r < m else 0
            passes = (d < x0[None]) | (x0[None] > 129)
            opened = [grp for grp in groups if passes[list(grp)].any()]    # the fold's maximum is the maximum of the group maxima
            if mode == "b":
                enter = sorted(i for grp in opened for i in grp)
            else:
                enter = sorted(i for grp in opened for i in grp if passes[i].any())
            if opened:
                fired.append((g0 // STAGE, g0 % STAGE // GROUP, tt))
                entered.append(tuple(enter))
                for i in enter:
                    for hk in range(2):
                        r = g0 + row_of(i, hk)
                        key = ((d[i, hk] << IDX_BITS) | r).astype(np.uint32) if r < hi else np.full(32, KEY_NONE, np.uint32)
                        lo2, hi2 = np.minimum(b1[tt, hk], b2[tt, hk]), np.maximum(b1[tt, hk], b2[tt, hk])
                        b2[tt, hk] = np.maximum(lo2, np.minimum(hi2, key))
                        b1[tt, hk] = np.minimum(b1[tt, hk], key)
                xs[tt] = np.minimum(xs[tt], (b2[tt] >> IDX_BITS).astype(np.int64))
            xs_log.append(xs[tt].copy())
    return b1, b2, np.array(xs_log), fired, entered


def tables(states):
    """The two smallest keys per query over the lanes of every worker."""
    keys = np.concatenate([np.stack([s[0][:, 0], s[0][:, 1], s[1][:, 0], s[1][:, 1]]).reshape(4, 64) for s in states])
    return np.sort(keys, axis=0)[:2]


def full_sort(dist):
    keys = ((dist.astype(np.int64) << IDX_BITS) | np.arange(len(dist))[:, None]).astype(np.uint32)
    return np.sort(keys, axis=0)[:2]


def random_case(seed, m=pipe.M):
    """Random descriptors, four warm rows per query family in the first group, and passing rows sprinkled at every index."""
    rng = np.random.default_rng(seed)
    q = rng.integers(0, 256, (64, 32), dtype=np.uint8)
    q[:] = q[0]
    q[7], q[40] = rng.integers(0, 256, (2, 32), dtype=np.uint8)
    t = rng.integers(0, 256, (m, 32), dtype=np.uint8)

    def at(row, d):
        bits = np.unpackbits(row)
        bits[rng.permutation(256)[:d]] ^= 1
        return np.packbits(bits)

    for j, base in ((0, 0), (7, 8), (40, 16)):
        for r, d in zip((0, 1, 4, 5), (40, 44, 46, 48)):
            t[base + r] = at(q[j], d)
    for i in range(16):                                                    # one passing row per index, in later groups
        t[64 + 32 * (i % 5) + row_of(i, i & 1)] = at(q[(0, 7, 40)[i % 3]], 20 + i)
    t[m - 1] = at(q[40], 3)                                                # and the last row of the ragged tail
    tb, qb = np.unpackbits(t, axis=1).astype(np.int64), np.unpackbits(q, axis=1).astype(np.int64)
    return tb @ (1 - qb).T + (1 - tb) @ qb.T


CASES = {name: hf.distances(a, b).T for name, (a, b) in pipe.FAMILIES.items()}
CASES["random_a"] = random_case(71)
CASES["random_b"] = random_case(72, 2 * STAGE + 5)
WORKERS = {"one": lambda m: [(0, m)], "many": lambda m: [(0, STAGE), (STAGE, 2 * STAGE), (2 * STAGE, m)]}


@pytest.mark.parametrize("workers", sorted(WORKERS))
@pytest.mark.parametrize("case", sorted(CASES))
def test_group_gates_then_row_gates_are_the_row_gates(case, workers):
    dist = CASES[case]
    for lo, hi in WORKERS[workers](len(dist)):
        old, new = replay(dist, "rows", lo=lo, hi=hi), replay(dist, "a", lo=lo, hi=hi)
        assert np.array_equal(old[0], new[0]) and np.array_equal(old[1], new[1]), "pairs"
        assert np.array_equal(old[2], new[2]), "thresholds after every group"
        assert old[3] == new[3] and len(new[3]) > 0, "fired (stage, group, tile)"
        assert old[4] == new[4], "entering rows"


@pytest.mark.parametrize("workers", sorted(WORKERS))
@pytest.mark.parametrize("case", sorted(CASES))
def test_whole_open_groups_give_the_full_sort(case, workers):
    dist = CASES[case]
    m = len(dist)
    states = []
    for lo, hi in WORKERS[workers](m):
        a, b = replay(dist, "a", lo=lo, hi=hi), replay(dist, "b", lo=lo, hi=hi)
        states.append(b)
        assert a[3] == b[3], "the same tiles fire: a fire is decided by the fold's maximum alone"
        assert all(set(x) <= set(y) for x, y in zip(a[4], b[4])), "a superset of the rows enters"
        assert (b[2] <= a[2]).all(), "a threshold is never looser"
        for keys in (b[0], b[1]):                                          # every published key is a real row's
            real = keys != KEY_NONE
            rows, col = (keys & np.uint32((1 << IDX_BITS) - 1)).astype(np.int64), np.broadcast_to(np.arange(32), keys.shape)
            q = col + 32 * np.arange(2)[:, None, None]
            assert (rows[real] >= lo).all() and (rows[real] < hi).all()
            assert np.array_equal((keys[real] >> IDX_BITS).astype(np.int64), dist[rows[real], q[real]])
    assert np.array_equal(tables(states), full_sort(dist))
    assert np.array_equal(tables([replay(dist, "a", lo=lo, hi=hi) for lo, hi in WORKERS[workers](m)]), full_sort(dist))


@pytest.mark.parametrize("mode", ["a", "b"])
def test_a_partition_that_leaves_an_index_out_is_caught(mode):
    for missing in range(16):
        dist = CASES["random_a"].copy()
        dist[2 * STAGE + row_of(missing, 1), 3] = 1                        # query 3's nearest sits at the index that is left out
        wrong = tuple(tuple(i for i in grp if i != missing) for grp in GATE_GROUPS)
        assert np.array_equal(tables([replay(dist, mode)]), full_sort(dist))
        got = replay(dist, mode, wrong)
        assert not np.array_equal(tables([got]), full_sort(dist)), missing
        assert got[4] != replay(dist, "rows")[4], missing


# ---- the built kernels ------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module", params=["bf_top2_mx32_kernel", "bf_mx32_image_top2_kernel"])
def kernel(request, built, tmp_path_factory):
    """(instructions in program order, metadata note) of one of the two kernels in the library the package loads."""
    if not (os.path.exists(OBJDUMP) and os.path.exists(READELF)):
        pytest.skip("llvm-objdump / llvm-readelf of the ROCm toolchain not found")
    from slamhip import _lib

    tmp = str(tmp_path_factory.mktemp("mx32_gates_isa"))
    local = os.path.join(tmp, "lib.so")
    shutil.copy(_lib.LIB_PATH, local)
    subprocess.run([OBJDUMP, "--offloading", local], cwd=tmp, check=True, capture_output=True)
    for f in sorted(os.listdir(tmp)):
        if "gfx950" not in f:
            continue
        obj = os.path.join(tmp, f)
        text = subprocess.run([OBJDUMP, "-d", obj], check=True, capture_output=True, text=True).stdout
        m = re.search(r"^[0-9a-f]+ <(_Z\d+" + request.param + r"\w*)>:$", text, re.M)
        if not m:
            continue
        body = text[m.end():].split("\n\n", 1)[0]
        ins = [ln.split("//")[0].strip() for ln in body.splitlines() if ln.split("//")[0].strip()]
        notes = subprocess.run([READELF, "--notes", obj], check=True, capture_output=True, text=True).stdout
        meta = next(b for b in re.split(r"\n\s+- \.agpr_count", notes) if re.search(r"\.name:\s+" + m.group(1) + r"\n", b))
        return ins, "\n    - .agpr_count" + meta
    pytest.fail(request.param + " is not in the library")


def field(meta, key):
    m = re.search(rf"\.{key}:\s+(\d+)", meta)
    assert m, key
    return int(m.group(1))


def test_the_limits_of_the_listing_tests_hold_for_both_kernels(kernel):
    ins, meta = kernel
    assert field(meta, "vgpr_count") + field(meta, "agpr_count") <= 128 and field(meta, "agpr_count") == 0
    for key in ("private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count"):
        assert field(meta, key) == 0, key
    assert field(meta, "group_segment_fixed_size") <= 40960
    assert not [s for s in ins if "scratch_" in s or "v_accvgpr_" in s]
    assert len([s for s in ins if s.startswith("v_max3_i32")]) >= 14
    assert not [s for s in ins if re.match(r"v_max3?_f32", s)]


def test_a_quiet_fold_is_eight_maxima_and_one_compare(kernel):
    ins, _ = kernel
    trips = pipe._trips(ins)
    assert len(trips) >= 2
    for trip in trips:
        folds = pipe._folds(ins, trip)
        assert len(folds) == 8
        for i, mine, _ in folds:
            end = next(k for k in range(i, i + 40) if ins[k].startswith("v_cmp_ge_i32_e32 vcc"))
            between = ins[i:end]
            assert len(between) == 8 and all(s.startswith(("v_max_i32", "v_max3_i32")) for s in between), between
            assert sum(s.startswith("v_max_i32") for s in between) == 1
            # the first level reads the tile's sixteen accumulators, each once
            read = [r for s in between for tok in s.split()[2:] for r in pipe._regs(tok.rstrip(",")) if r in mine]
            assert sorted(read) == sorted(mine)


def test_a_fired_block_tests_no_more_gates_at_once_than_there_are_groups(kernel):
    """The gate compares stand back to back into SGPR pairs in front of the scalar tests.  A run of them, up to the first scalar
    compare or branch, was 16 long with the row gates; now it is the group gates' five (and never more)."""
    ins, _ = kernel
    runs, cur = [], 0
    for s in ins:
        if re.match(r"v_cmp_ge_i32_e64 s\[\d+:\d+\]", s):
            cur += 1
        elif s.startswith(("s_cmp", "s_cbranch", "s_branch")):
            if cur:
                runs.append(cur)
            cur = 0
    assert runs and max(runs) == len(GATE_GROUPS), sorted(set(runs))
    assert runs.count(len(GATE_GROUPS)) >= 16, "every fold of both trips has its fired block"
