"""CPU suite: what the overlapped scan loop of the matrix-core top-2 search (bf_mx.hip: operand reads and staging behind the
MFMAs) must leave as it was - the block's LDS footprint, on the built library's gfx950 code object the way
tests/test_mx_isa_cpu.py reads it, and the plan that slam_bf_mx_plan_describe reports.

`expected_plan` restates the planner's documented rule (the comment over make_mx_plan_core): workers = CUs x 4 resident
blocks / query blocks, in [1, 256] and at most one per chunk; chunks of 1024 rows where a worker has at least 8192 rows to
itself, 256 below; from the point where the rest would give every worker fewer than two of those, (rest / 2 workers) rows
rounded down to whole 128-row stages, never fewer than one stage.  tests/test_mx_overlap_gpu.py asserts its plans with it."""
import os
import re
import shutil
import subprocess

import pytest

LLVM = "/opt/rocm/lib/llvm/bin"
OBJDUMP = os.path.join(LLVM, "llvm-objdump")
READELF = os.path.join(LLVM, "llvm-readelf")
STAGE, RESIDENT = 128, 4
LDS_PER_CU = 160 * 1024


def expected_plan(num_cu, n, m):
    """(plan dict, chunk boundary table) by the documented rule, in integers."""
    qblocks = (n + 255) // 256
    w = min(max(num_cu * RESIDENT // qblocks, 1), 256)
    c = 1024 if m // w >= 8192 else 256
    tbl, tail, at = [0], 0, 0
    while at < m:
        ln = c
        g = (m - at) // (2 * w) // STAGE * STAGE
        if g < ln:
            ln = max(g, STAGE)
            tail += 1
        at = min(at + ln, m)
        tbl.append(at)
    chunks = len(tbl) - 1
    auto = (n >= 8192 and m >= 16384) or (n >= 3000 and m >= 40000) or (n >= 1000 and m >= 65536) or (n >= 500 and m >= 200000)
    return dict(qblocks=qblocks, workers=min(w, chunks), chunk=c, chunks=chunks, tail_chunks=tail, stage_rows=STAGE,
                resident=RESIDENT, auto=int(auto)), tbl


def test_block_lds_leaves_four_blocks_per_cu(built, tmp_path):
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
                # two expanded stages of 16 KiB at the least; a quarter of the CU's LDS at the most (RESIDENT blocks per CU)
                assert 2 * STAGE * 128 <= lds <= LDS_PER_CU // RESIDENT == 40960, lds
                return
    pytest.fail("bf_top2_mx_kernel is not in the library")


SHAPES = [(256, 65536, 65536), (256, 8192, 65536), (256, 8192, 16384), (256, 3000, 40000), (256, 1000, 65536),
          (256, 500, 200000), (256, 64, 127), (256, 64, 128), (256, 300, 1151), (256, 16384, 16384 + 77), (256, 65536, 32768),
          (304, 65536, 65536), (80, 4096, 100000), (1, 70, 5000)]


@pytest.mark.parametrize("num_cu,n,m", SHAPES)
def test_plan_describe_is_the_documented_rule(built, num_cu, n, m):
    import slamhip

    p, tbl = slamhip.mx_plan_describe(n, m, num_cu=num_cu)
    want, wtbl = expected_plan(num_cu, n, m)
    assert p == want
    assert tbl == wtbl
    assert p["stage_rows"] == 128 and p["resident"] == 4


def test_the_bench_shape_runs_chunks_of_eight_stages(built):
    """65536 x 65536 on 256 CUs: 4 workers per query block and 1024-row chunks - seven of a chunk's eight stages are whole
    stages that another follows, the ones whose shadow carries the next stage's staging."""
    import slamhip

    p, tbl = slamhip.mx_plan_describe(65536, 65536, num_cu=256)
    assert (p["qblocks"], p["workers"], p["chunk"], p["auto"]) == (256, 4, 1024, 1)
    assert tbl[:3] == [0, 1024, 2048] and tbl[-1] == 65536
