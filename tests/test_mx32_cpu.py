"""CPU suite: the 32x32x64 matrix-core top-2 search (bf_mx32.hip) without a GPU - its expand / K map and the row order of its
lane map restated in numpy, the form of the kernel in the built library's gfx950 code object (the unscaled FP4 32x32x64
MFMA only, accumulators in VGPRs, the registers of four waves per SIMD, no scratch, the LDS of four blocks per CU), and the
routing between the two matrix-core kernels against its documented rule."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

LLVM = "/opt/rocm/lib/llvm/bin"
OBJDUMP = os.path.join(LLVM, "llvm-objdump")
READELF = os.path.join(LLVM, "llvm-readelf")


# ---- the maps -----------------------------------------------------------------------------------------------------------

def expand(x):
    """mx_expand (bf_mx_common.h) on uint32 words -> [..., 4] uint32: nibble n of output word w = FP4 -1.0 (0xA) if bit 4n + w
    of the source word is set, else +1.0 (0x2)."""
    x = np.asarray(x, np.uint32)
    return np.stack([((x << np.uint32(3 - w)) & np.uint32(0x88888888)) | np.uint32(0x22222222) for w in range(4)], -1)


def fp4_values(words):
    """[..., k] uint32 of FP4 nibbles 0x2 / 0xA -> [..., 8 k] of +1 / -1."""
    nib = (words[..., None] >> (4 * np.arange(8, dtype=np.uint32))) & np.uint32(0xF)
    assert np.isin(nib, (0x2, 0xA)).all()
    return np.where(nib == 0xA, -1, 1).reshape(*words.shape[:-1], -1)


def operand(rows):
    """rows [32, 8] uint32 -> the A (or B) operands of the four K-quarters: [4, 64 lanes, 4 words].  Lane (row & 31) + 32 hk of
    quarter q holds the expansion of source word 2 q + hk."""
    out = np.empty((4, 64, 4), np.uint32)
    for q in range(4):
        for hk in range(2):
            out[q, 32 * hk:32 * hk + 32] = expand(rows[:, 2 * q + hk])
    return out


def mfma_32x32x64(a, b):
    """D[i][j] of v_mfma_f32_32x32x64 for FP4 operands [64 lanes, 4 words]: lane l of A holds row l & 31, of B column l & 31,
    K values 32 (l >> 5) .. + 31."""
    av, bv = fp4_values(a), fp4_values(b)                        # [64, 32]
    d = np.zeros((32, 32), np.int64)
    for hk in range(2):
        d += av[32 * hk:32 * hk + 32] @ bv[32 * hk:32 * hk + 32].T
    return d


def popcount_dist(q, t):
    x = q[:, None, :] ^ t[None, :, :]
    return np.unpackbits(x.view(np.uint8), axis=-1).sum(-1)


EDGE_ROWS = [np.zeros(8, np.uint32), np.full(8, 0xFFFFFFFF, np.uint32), np.full(8, 0x80000001, np.uint32),
             np.arange(8, dtype=np.uint32), np.full(8, 0x0F0F0F0F, np.uint32), np.array([1, 0, 0, 0, 0, 0, 0, 1 << 31], np.uint32)]


def test_expand_keeps_every_bit_once():
    rng = np.random.default_rng(1)
    x = np.concatenate([rng.integers(0, 1 << 32, 500, dtype=np.uint64).astype(np.uint32), np.array([0, 0xFFFFFFFF, 1, 1 << 31], np.uint32)])
    v = fp4_values(expand(x))                                    # [n, 32]
    bits = (x[:, None] >> np.arange(32, dtype=np.uint32)) & 1
    # element 8 w + n of the expansion is bit 4 n + w
    w, n = np.divmod(np.arange(32), 8)
    assert np.array_equal(v, np.where(bits[:, 4 * n + w] == 1, -1, 1))


def test_dot_over_four_quarters_is_the_hamming_distance():
    rng = np.random.default_rng(2)
    q = rng.integers(0, 1 << 32, (32, 8), dtype=np.uint64).astype(np.uint32)
    t = rng.integers(0, 1 << 32, (32, 8), dtype=np.uint64).astype(np.uint32)
    t[:len(EDGE_ROWS)] = EDGE_ROWS
    q[5], q[6], q[7] = t[0], ~t[1], t[2] ^ np.uint32(1)
    a, b = operand(t), operand(q)
    d = sum(mfma_32x32x64(a[kq], b[kq]) for kq in range(4))      # D[train row][query]
    assert np.array_equal((256 - d) // 2, popcount_dist(t, q)) and (d % 2 == 0).all()


def test_lane_map_rows_ascend_with_the_accumulator_index():
    # lane l, accumulator index 4 i + j -> row 8 i + 4 (l >> 5) + j: the two lanes of a query hold every row of the group once,
    # and each lane's rows ascend with the index (the tie rules merge a lane's rows in index order)
    rows = np.array([[8 * (k >> 2) + 4 * hk + (k & 3) for k in range(16)] for hk in range(2)])
    assert (np.diff(rows, axis=1) > 0).all()
    assert sorted(rows.ravel().tolist()) == list(range(32))


def test_fold_compare_is_exact_where_it_is_trusted():
    """The fold compares bit patterns as signed integers against the pattern of 258 - 2 x (x <= 129), INT_MIN above: for every
    even dot in [-256, 256] and every x that must say dist < x, or fire."""
    d = np.arange(-256, 257, 2).astype(np.float32)
    pat = d.view(np.int32)
    for x in range(0, 512):
        thr = np.int32(-2 ** 31) if x > 129 else np.float32(258 - 2 * x).view(np.int32)
        passes = pat >= thr
        exact = (256 - d) / 2 < x
        assert np.array_equal(passes, exact) if x <= 129 else passes.all(), x


# ---- the built kernel ---------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def mx32_kernel(built, tmp_path_factory):
    """(disassembly of bf_top2_mx32_kernel, its metadata note) from the library the package loads."""
    if not (os.path.exists(OBJDUMP) and os.path.exists(READELF)):
        pytest.skip("llvm-objdump / llvm-readelf of the ROCm toolchain not found")
    from slamhip import _lib

    tmp = str(tmp_path_factory.mktemp("mx32_isa"))
    local = os.path.join(tmp, "lib.so")
    shutil.copy(_lib.LIB_PATH, local)
    subprocess.run([OBJDUMP, "--offloading", local], cwd=tmp, check=True, capture_output=True)
    for f in sorted(os.listdir(tmp)):                               # one gfx950 code object per source file
        if "gfx950" not in f:
            continue
        obj = os.path.join(tmp, f)
        text = subprocess.run([OBJDUMP, "-d", obj], check=True, capture_output=True, text=True).stdout
        m = re.search(r"^[0-9a-f]+ <(_Z\d+bf_top2_mx32_kernel\w*)>:$", text, re.M)
        if not m:
            continue
        body = text[m.end():].split("\n\n", 1)[0]
        notes = subprocess.run([READELF, "--notes", obj], check=True, capture_output=True, text=True).stdout
        meta = next(b for b in re.split(r"\n\s+- \.agpr_count", notes) if re.search(r"\.name:\s+" + m.group(1) + r"\n", b))
        return body, "\n    - .agpr_count" + meta
    pytest.fail("bf_top2_mx32_kernel is not in the library")


def field(meta, key):
    m = re.search(rf"\.{key}:\s+(\d+)", meta)
    assert m, f"no .{key} in the kernel's metadata"
    return int(m.group(1))


def test_every_mfma_is_the_fp4_32x32x64_form(mx32_kernel):
    body, _ = mx32_kernel
    mfma = [ln.split("//")[0].strip() for ln in body.splitlines() if "v_mfma" in ln]
    assert len(mfma) >= 8
    for ln in mfma:
        assert re.search(r"v_mfma(_scale)?_f32_32x32x64_f8f6f4 .* cbsz:4 blgp:4", ln), ln
    # the shipped spelling is the unscaled one, and a tile's first K-quarter starts from the inline constant 0
    assert not [ln for ln in mfma if "_scale_" in ln]
    assert [ln for ln in mfma if re.search(r"\], 0 cbsz:4", ln)]


def test_accumulators_stay_in_vgprs(mx32_kernel):
    body, meta = mx32_kernel
    assert "v_accvgpr_" not in body
    assert field(meta, "agpr_count") == 0
    mfma = [ln for ln in body.splitlines() if "v_mfma" in ln]
    assert not any(re.search(r"\ba\[?\d", ln.split("v_mfma", 1)[1].split("//")[0]) for ln in mfma), mfma[:2]


def test_four_waves_per_simd_no_scratch_and_lds_of_four_blocks(mx32_kernel):
    body, meta = mx32_kernel
    assert field(meta, "vgpr_count") + field(meta, "agpr_count") <= 128
    assert "scratch_" not in body
    for key in ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size"):
        assert field(meta, key) == 0, key
    assert field(meta, "group_segment_fixed_size") <= 40960


def test_fold_is_integer(mx32_kernel):
    body, _ = mx32_kernel
    assert len([ln for ln in body.splitlines() if "v_max3_i32" in ln]) >= 14
    assert not [ln for ln in body.splitlines() if re.search(r"v_max3?_f32", ln)]


# ---- routing ------------------------------------------------------------------------------------------------------------

def rule(n, m):
    """DESIGN.md 3c "The 32x32x64 kernel", routing table: the shapes that engine 0 runs on the 32x32x64 kernel, among those it
    sends to the matrix cores at all: at most 131072 queries and at most 200000 train rows."""
    return n <= 131072 and m <= 200000


def test_routing_follows_the_documented_rule(built):
    import slamhip

    for n in (1, 500, 999, 1000, 2999, 3000, 8191, 8192, 20000, 65536, 131072, 131073, 1 << 20):
        for m in (1, 16383, 16384, 39999, 40000, 65535, 65536, 100000, 199999, 200000, 200001, 1 << 20, 1 << 23):
            assert slamhip.mx_tile_describe(n, m, 0) == (32 if rule(n, m) else 16), (n, m)
            assert slamhip.mx_tile_describe(n, m, 2) == 16
            assert slamhip.mx_tile_describe(n, m, 3) == 32


def test_engine_3_is_accepted_and_4_is_not(built):
    import slamhip
    from slamhip._lib import SlamHipError

    assert slamhip.mx_tile_describe(4096, 4096, 3) == 32
    for engine in (1, 4, -1):
        with pytest.raises(SlamHipError):
            slamhip.mx_tile_describe(4096, 4096, engine)
