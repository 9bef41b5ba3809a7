"""CPU suite: the matrix-core top-2 search (bf_mx.hip) without a GPU - the +-1 FP4 encoding and the identity it rests on,
the invariants of its planner (slam_bf_mx_plan_describe), and the instruction it is built around, on the built library's
gfx950 code object."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
FP4 = {0x2: 1.0, 0xA: -1.0}


def mx_expand(words: np.ndarray) -> np.ndarray:
    """bf_mx.hip mx_expand on uint32 words -> [..., 4] uint32: nibble n of word w = FP4 +1 (0x2) if bit 4n + w is set, else
    -1 (0xA)."""
    n = ~words.astype(np.uint32)
    out = []
    for w in range(4):
        sh = (n << np.uint32(3 - w)) if w < 3 else n
        out.append((sh & np.uint32(0x88888888)) | np.uint32(0x22222222))
    return np.stack(out, axis=-1).astype(np.uint32)


def fp4_values(expanded: np.ndarray) -> np.ndarray:
    """The E2M1 values of the nibbles of expanded words (every nibble must be +1 or -1)."""
    nib = np.stack([(expanded >> np.uint32(4 * i)) & np.uint32(0xF) for i in range(8)], axis=-1).reshape(*expanded.shape[:-1], -1)
    assert set(np.unique(nib).tolist()) <= set(FP4), np.unique(nib)
    return np.where(nib == 0x2, 1.0, -1.0)


def pm1(rows: np.ndarray) -> np.ndarray:
    """[n, 32] uint8 descriptors -> [n, 256] +-1 in the kernel's K order (both operands use the same map)."""
    return fp4_values(mx_expand(rows.view("<u4"))).reshape(len(rows), -1)


def hamming(a, b):
    return np.unpackbits(a[:, None, :] ^ b[None, :, :], axis=-1).sum(-1).astype(np.int64)


def test_expansion_is_a_bijection_of_the_bits():
    rng = np.random.default_rng(1)
    w = rng.integers(0, 2 ** 32, 4096, dtype=np.uint64).astype(np.uint32)
    v = fp4_values(mx_expand(w))                                   # [4096, 32]
    bits = ((w[:, None] >> np.arange(32, dtype=np.uint32)) & 1).astype(np.int64)
    # element 8 w + n of the word's 32 is bit 4 n + w
    perm = np.array([4 * n + k for k in range(4) for n in range(8)])
    assert np.array_equal(v, np.where(bits[:, perm] == 1, 1.0, -1.0))
    assert sorted(perm.tolist()) == list(range(32))


@pytest.mark.parametrize("kind", ["random", "edges"])
def test_dot_identity(kind):
    rng = np.random.default_rng(7)
    if kind == "random":
        a = rng.integers(0, 256, (200, 32), dtype=np.uint8)
        b = rng.integers(0, 256, (300, 32), dtype=np.uint8)
    else:
        a = np.array([[0] * 32, [255] * 32, [0xAA] * 32, [0x55] * 32, [1] + [0] * 31, [0] * 31 + [128]], np.uint8)
        b = a.copy()
    dot = pm1(a) @ pm1(b).T
    h = hamming(a, b)
    assert np.array_equal(256 - 2 * h, dot)
    # the accumulator starts at 2 d2 - 256 and the kernel reads the distance back as d2 - D / 2
    for d2 in (0, 37, 128, 256, 511):
        D = dot + (2 * d2 - 256)
        assert np.all(D % 2 == 0) and np.array_equal(d2 - D // 2, h)
        assert np.array_equal(D >= 0, h <= d2)
        assert np.abs(D).max() <= 256 + 1022                     # exact in f32


def describe(n, m, num_cu=256):
    import slamhip

    return slamhip.mx_plan_describe(n, m, num_cu=num_cu)


@pytest.mark.parametrize("n,m", [(65536, 65536), (8192, 65536), (1, 16384), (257, 769), (1000, 5001), (700, 70001),
                                 (131072, 1 << 20), (16384, 1 << 23), (300, 17)])
@pytest.mark.parametrize("num_cu", [256, 80, 1])
def test_mx_plan_invariants(built, n, m, num_cu):
    p, tbl = describe(n, m, num_cu)
    assert p["qblocks"] == (n + 255) // 256
    assert p["stage_rows"] == 128 and p["resident"] >= 1
    assert len(tbl) == p["chunks"] + 1 and tbl[0] == 0 and tbl[-1] == m
    sizes = np.diff(tbl)
    assert np.all(sizes > 0)
    assert np.all(sizes[:-1] % p["stage_rows"] == 0)                # every chunk but the last starts on a stage boundary
    assert np.all(sizes <= p["chunk"]) and p["chunk"] % p["stage_rows"] == 0
    assert 1 <= p["workers"] <= min(256, p["chunks"])
    assert p["workers"] <= max(1, num_cu * p["resident"] // p["qblocks"])
    assert 0 <= p["tail_chunks"] <= p["chunks"]
    assert p["chunks"] + 1 <= 65536


def test_mx_auto_shapes(built):
    assert describe(65536, 65536)[0]["auto"] == 1
    assert describe(8192, 65536)[0]["auto"] == 1
    assert describe(200, 200)[0]["auto"] == 0
    assert describe(4096, 4096)[0]["auto"] == 0
    # measured slower there (profiles/r05_mx_sweep.log): stays on the VALU kernel
    for n, m in ((2048, 16384), (2048, 40000), (3000, 24000), (500, 100000), (1000, 40000)):
        assert describe(n, m)[0]["auto"] == 0, (n, m)
    for n, m in ((500, 1000000), (1000, 65536), (3000, 40000), (8192, 16384), (262144, 1000000)):
        assert describe(n, m)[0]["auto"] == 1, (n, m)
    # one step inside and one outside each clause of bf_mx_auto (tests/test_mx_edges_gpu.py runs these shapes)
    for n, m in ((8191, 16384), (8192, 16383), (2999, 40000), (3000, 39999), (999, 65536), (1000, 65535), (499, 200000),
                 (500, 199999), (499, 1 << 23), (130, 1 << 23), (640, 777), (65536, 16383)):
        assert describe(n, m)[0]["auto"] == 0, (n, m)
    for n, m in ((8192, 16384), (3000, 40000), (1000, 65536), (500, 200000), (640, 1 << 23), (8229, 16384), (65537, 30001),
                 ((1 << 18) + 3, 16384), (1000, 150001)):
        assert describe(n, m)[0]["auto"] == 1, (n, m)


def test_describe_refuses_bad_sizes(built):
    import slamhip

    with pytest.raises(slamhip.SlamHipError):
        describe(0, 100)
    with pytest.raises(slamhip.SlamHipError):
        describe(100, (1 << 23) + 1)


def test_kernel_is_built_on_the_fp4_mfma(built, tmp_path):
    if not os.path.exists(OBJDUMP):
        pytest.skip("llvm-objdump of the ROCm toolchain not found")
    from slamhip import _lib

    local = os.path.join(str(tmp_path), "lib.so")
    shutil.copy(_lib.LIB_PATH, local)
    subprocess.run([OBJDUMP, "--offloading", local], cwd=str(tmp_path), check=True, capture_output=True)
    body = meta = None
    for f in sorted(os.listdir(str(tmp_path))):                     # one gfx950 code object per source file
        if "gfx950" not in f:
            continue
        obj = os.path.join(str(tmp_path), f)
        text = subprocess.run([OBJDUMP, "-d", obj], check=True, capture_output=True, text=True).stdout
        m = re.search(r"^[0-9a-f]+ <(_Z\d+bf_top2_mx_kernel\w*)>:$", text, re.M)
        if m:
            body = text[m.end():].split("\n\n", 1)[0]
            notes = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-readelf", "--notes", obj], check=True, capture_output=True,
                                   text=True).stdout
            meta = next(b for b in re.split(r"\n\s+- \.agpr_count", notes) if re.search(r"\.name:\s+" + m.group(1) + r"\n", b))
            break
    assert body is not None, "bf_top2_mx_kernel is not in the library"
    mfma = [ln for ln in body.splitlines() if "v_mfma" in ln]
    assert len(mfma) >= 8 and all(re.search(r"v_mfma_scale_f32_16x16x128_f8f6f4 .* cbsz:4 blgp:4", ln) for ln in mfma), mfma[:2]
    assert "scratch_" not in body, "the MX kernel spills"
    for key in ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size"):
        m = re.search(rf"\.{key}:\s+(\d+)", meta)
        assert m and int(m.group(1)) == 0, (key, m and m.group(0))
